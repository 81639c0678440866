"""Worker of tests/test_optimizers_gpu.py::test_rmsprop_clipnorm_two_ranks_equal_one_rank: the CNN point estimator trained with
RMSprop + clipnorm on the real HIP path, every rank on cuda:0 over gloo (torch.distributed.run with WORLD_SIZE ranks, or directly as the
single-process reference).  Writes losses, final weights and the clip factor of every step to argv[1].<rank>."""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def main(out):
    import torch
    from gennet_amd import bbh, dist, engine
    dp = dist.init('gloo')
    rank, world = (dp.rank, dp.world_size) if dp else (0, 1)
    engine.set_init_seed(7)
    n_pix, B = 64, 8
    lo, hi = rank * B // world, (rank + 1) * B // world
    rng = np.random.RandomState(17)
    PE = bbh.signal_pe_model(n_pix)
    PE.compile(loss='mean_squared_error', optimizer=engine.RMSprop(lr=1e-4, clipnorm=1.0), metrics=['accuracy'], data_parallel=dp)
    res = {'losses': [], 'factor': []}
    for _ in range(4):
        x = f32(rng.randn(B, n_pix, 1)); ymc = f32(rng.uniform(20, 35, B)); yq = f32(rng.uniform(0.5, 1, B))
        res['losses'].append(PE.train_on_batch(x[lo:hi], [ymc[lo:hi], yq[lo:hi]]))
        res['factor'].append(PE.optimizer._factor.cpu().numpy().copy())
    res['weights'] = PE.get_weights()
    pickle.dump(res, open('%s.%d' % (out, rank), 'wb'))
    if dp:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
