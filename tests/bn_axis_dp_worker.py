"""Worker of tests/test_bn_axis_gpu.py's data-parallel test: the sibling-discriminator stack (Conv1D(tanh) -> LeakyReLU -> BatchNormalization(axis=1),
twice, Flatten, Dense) at global batch 8 for three SGD steps, N ranks x 8/N rows on cuda:0 over gloo, or one rank x 8 rows without a process
group.  The statistics of both BatchNormalization layers and their backward sums are all-reduced (count x world size), so the ranks reproduce
the single-process batch.  Writes {'losses', 'weights'} to argv[1].<rank>."""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def discriminator(moving_average=None):
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Sequential
    return Sequential([Ly.Reshape((-1, 1), input_shape=(64,)), Ly.Conv1D(6, 8, padding='valid', activation='tanh'), Ly.LeakyReLU(0.2),
                       Ly.BatchNormalization(axis=1, moving_average=moving_average), Ly.Conv1D(12, 8, padding='valid', activation='tanh'), Ly.LeakyReLU(0.2),
                       Ly.BatchNormalization(axis=1, moving_average=moving_average), Ly.Flatten(), Ly.Dense(2, activation='sigmoid')])


def run(out):
    import torch
    from gennet_amd import dist, engine
    from gennet_amd.engine import SGD
    dp = dist.init('gloo')
    rank, world = (dp.rank, dp.world_size) if dp else (0, 1)
    engine.set_init_seed(21)
    B = 8
    lo, hi = rank * B // world, (rank + 1) * B // world
    rng = np.random.RandomState(4)
    model = discriminator()
    for l in model.layers:
        if l.__class__.__name__ == 'BatchNormalization':
            P = l.view[1]
            l.set_weights([1 + 0.2 * rng.randn(P), 0.2 * rng.randn(P), 0.3 * rng.randn(P), 0.5 + rng.rand(P)])
    model.compile(optimizer=SGD(lr=0.05), loss='mean_squared_error', data_parallel=dp)
    res = {'losses': []}
    for it in range(3):
        x = rng.randn(B, 64).astype(np.float32); t = rng.rand(B, 2).astype(np.float32)
        res['losses'].append(float(np.ravel(model.train_on_batch(x[lo:hi], t[lo:hi]))[0]))
    res['weights'] = model.get_weights()
    pickle.dump(res, open('%s.%d' % (out, rank), 'wb'))
    if dp:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    run(sys.argv[1])
