"""Worker of the data-parallel sample-weight test (tests/test_sample_weight_gpu.py), started as tests/dp_worker.py's `gpu` mode is: by
torch.distributed.run with two ranks on cuda:0 (gloo over CUDA tensors), or directly as the one-rank reference.

A small Dense net with a (B, 3) logcosh head and a (B, 1) binary_crossentropy head trains on B = 8 rows, rank r on rows [r B / N, (r + 1) B / N).
The first head's weights are mixed on rank 0's rows (a zero and a negative one among them) and ALL ZERO on rank 1's; the second head's entry is
None.  The number of non-zero weights is a global quantity: a rank that divided by its local count would divide rank 1's sums by zero.
Writes {'losses', 'weights', 'calls_weighted', 'calls_unweighted'} to argv[1].<rank>."""
import os
import pickle
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out):
    from gennet_amd import dist, engine, layers
    dp = dist.init('gloo')
    rank, world = (dp.rank, dp.world_size) if dp else (0, 1)
    B = 8
    lo, hi = rank * B // world, (rank + 1) * B // world
    rng = np.random.RandomState(21)
    x = engine.Input(shape=(16,))
    h = layers.Dense(8, activation='tanh')(x)
    m = engine.Model(inputs=x, outputs=[layers.Dense(3, activation='sigmoid')(h), layers.Dense(1, activation='sigmoid')(h)])
    m.set_weights([(0.5 * rng.randn(*w.shape)).astype(np.float32) for w in m.get_weights()])
    m.compile(loss=['logcosh', 'binary_crossentropy'], optimizer=engine.Adam(lr=9e-5), loss_weights=[1.0, 0.5], metrics=['accuracy'],
              weighted_metrics=['accuracy', 'mae'], data_parallel=dp)
    xs = rng.randn(B, 16).astype(np.float32)
    ys = [rng.uniform(0.1, 0.9, (B, 3)).astype(np.float32), rng.randint(0, 2, (B, 1)).astype(np.float32)]
    sw = np.array([2.0, 0.0, -0.5, 1.25, 0.0, 0.0, 0.0, 0.0], np.float32)
    res = {'losses': []}

    def step(weighted):
        if dp:
            dp.reset_counters()
        r = m.train_on_batch(xs[lo:hi], [y[lo:hi] for y in ys], sample_weight=[sw[lo:hi], None] if weighted else None)
        res['losses'].append(r)
        return dp.calls if dp else 0
    step(True)                                       # binds the flat gradient buffers: from here on the number of segments is fixed
    res['calls_weighted'] = step(True)
    res['calls_unweighted'] = step(False)
    res['losses'].append(m.test_on_batch(xs[lo:hi], [y[lo:hi] for y in ys], sample_weight=[sw[lo:hi], None]))
    res['weights'] = m.get_weights()
    pickle.dump(res, open('%s.%d' % (out, rank), 'wb'))
    if dp:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
