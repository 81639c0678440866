#!/usr/bin/env python
"""python tests/golden/make_h5_golden.py DIR  (DIR: the four real Keras 2.1.6 files the reference ships, 2_model_version/weight_version/*.hdf5)

Writes tests/golden/keras_h5_golden.json: names, shapes, dtypes and CRC32s of everything in the four files, read with gennet_amd/h5lite.py.
That JSON holds no weights and no reference text; model_config / training_config -- the JSON Keras ITSELF wrote into the two full-model
files, i.e. Keras' own record of its layer and optimizer defaults (BatchNormalization epsilon / momentum / initialisers, LeakyReLU alpha,
the glorot VarianceScaling spec, Adam beta_2 / epsilon stored as float32 variables) -- are recorded in full as parsed JSON ('model_config',
'training') next to the structure summary ('model').

Writes the files themselves under tests/golden/keras_h5/: a file of at most MAX_BYTES unchanged; a larger one (the two full-model files,
whose Adam moments triple the weights) as <name>.gz with the raw data of every float32 dataset of more than FILL_MIN bytes set to zero,
the zeroed regions listed in keras_h5/filled.json as [dataset path, byte offset, byte count].  Superblock, object headers, B-trees, heaps,
attributes and the small datasets (biases, Adam scalars, the iteration count) keep the file's own bytes.  tests/test_h5.py rebuilds such
a file with every zeroed float32 word holding its own byte offset (fill_words), so a reader that reads from the wrong place still fails.
"""
import gzip
import importlib.util
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'keras_h5')
MAX_BYTES = 1 << 20
FILL_MIN = 4096
spec = importlib.util.spec_from_file_location('h5lite', os.path.join(HERE, '..', '..', 'gennet_amd', 'h5lite.py'))
h5lite = importlib.util.module_from_spec(spec)
spec.loader.exec_module(h5lite)


def fill_words(off, nbytes):
    """float32 words whose values are their own byte offsets in the file (exact below 2**24)."""
    return np.arange(off, off + nbytes, 4, dtype=np.int64).astype('<f4').tobytes()


def reduce_file(raw):
    """(the bytes with the large float32 datasets zeroed, [[path, offset, nbytes], ...]); checks that every region is found exactly once
    and that the rebuilt file reads back fill_words there and the original bytes everywhere else."""
    f = h5lite.File(raw)
    buf = bytearray(raw)
    regions = []
    for path, o in f.visit():
        if not isinstance(o, h5lite.Dataset) or o.dtype != np.float32:
            continue
        b = np.ascontiguousarray(o.value).tobytes()
        if len(b) <= FILL_MIN:
            continue
        off = raw.find(b)
        assert off >= 0 and raw.find(b, off + 1) < 0 and off + len(b) < 1 << 24, path      # contiguous, unfiltered, found once
        buf[off:off + len(b)] = bytes(len(b))
        regions.append([path, off, len(b)])
    rebuilt = bytearray(buf)
    for path, off, n in regions:
        rebuilt[off:off + n] = fill_words(off, n)
    g = h5lite.File(bytes(rebuilt))
    for path, off, n in regions:
        assert np.ascontiguousarray(g[path].value).tobytes() == fill_words(off, n), path
    assert h5lite.dump_structure(bytes(rebuilt))['attrs'] == h5lite.dump_structure(raw)['attrs']
    return bytes(buf), regions


if __name__ == '__main__':
    src = sys.argv[1]
    out, filled = {}, {}
    os.makedirs(OUT, exist_ok=True)
    for fn in ('d_model.hdf5', 'g_model.hdf5', 'best_d_weights.hdf5', 'best_g_weights.hdf5'):
        raw = open(os.path.join(src, fn), 'rb').read()
        d = h5lite.dump_structure(raw)
        f = h5lite.File(raw)
        d['file_bytes'] = len(raw)
        mc = f.attrs.get('model_config')
        if mc is not None:
            cfg = json.loads(mc)
            d['model'] = {'class_name': cfg['class_name'], 'name': cfg['config']['name'],
                          'layers': [[l['class_name'], l['name']] for l in cfg['config']['layers']]}
            d['model_config'] = cfg
            d['training'] = json.loads(f.attrs['training_config'])
        out[fn] = d
        if len(raw) <= MAX_BYTES:
            open(os.path.join(OUT, fn), 'wb').write(raw)
            continue
        zeroed, regions = reduce_file(raw)
        for path, off, n in regions:                      # the regions hold exactly the datasets the golden JSON describes
            assert zlib.crc32(raw[off:off + n]) & 0xFFFFFFFF == d['datasets'][path][2], path
        open(os.path.join(OUT, fn + '.gz'), 'wb').write(gzip.compress(zeroed, 9, mtime=0))
        filled[fn] = regions
    json.dump(out, open(os.path.join(HERE, 'keras_h5_golden.json'), 'w'), indent=1, sort_keys=True)
    json.dump(filled, open(os.path.join(OUT, 'filled.json'), 'w'), indent=1, sort_keys=True)
    print('wrote', {k: (len(v['datasets']), len(v['groups'])) for k, v in out.items()}, {k: len(v) for k, v in filled.items()})
