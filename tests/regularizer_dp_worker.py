"""Worker of the data-parallel regularizer test (tests/test_regularizers_gpu.py), started as tests/sample_weight_dp_worker.py is: by
torch.distributed.run with two ranks (gloo over CUDA tensors), or directly as the one-rank reference.

A small Dense net with weight regularizers on both layers and activity regularizers on the hidden layer (the keyword) and behind the head (an
ActivityRegularization layer) trains on B = 8 rows for three Adam steps, rank r on rows [r B / N, (r + 1) B / N), then runs one test step.  The
weight penalties are a property of the replicated weights: they enter the loss once, not once per rank, and their gradient is added once to the
all-reduced gradient.  The activity penalties are sums over the global batch: every rank holds the sum of its own rows.
Writes {'losses', 'weights', 'penalty_share'} to argv[1].<rank>."""
import os
import pickle
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out):
    from gennet_amd import dist, engine, layers, regularizers
    dp = dist.init('gloo')
    rank, world = (dp.rank, dp.world_size) if dp else (0, 1)
    B = 8
    lo, hi = rank * B // world, (rank + 1) * B // world
    rng = np.random.RandomState(23)

    def build(regs):
        kw1 = dict(kernel_regularizer=regularizers.l1_l2(0.01, 0.02), bias_regularizer=regularizers.l2(0.1),
                   activity_regularizer=regularizers.l1(0.001)) if regs else {}
        kw2 = dict(kernel_regularizer=regularizers.l2(0.01)) if regs else {}
        return engine.Sequential([layers.Dense(8, activation='tanh', input_shape=(16,), **kw1), layers.Dense(3, **kw2)]
                                 + ([layers.ActivityRegularization(l2=0.02)] if regs else []))
    m, plain = build(True), build(False)
    m.set_weights([(0.5 * rng.randn(*w.shape)).astype(np.float32) for w in m.get_weights()])
    plain.set_weights(m.get_weights())
    m.compile(loss='mean_squared_error', optimizer=engine.Adam(lr=9e-5), data_parallel=dp)
    plain.compile(loss='mean_squared_error', optimizer=engine.Adam(lr=9e-5), data_parallel=dp)
    xs, ys = rng.randn(B, 16).astype(np.float32), rng.randn(B, 3).astype(np.float32)
    bare = float(np.ravel(plain.test_on_batch(xs[lo:hi], ys[lo:hi]))[0])
    res = {'losses': [float(np.ravel(m.train_on_batch(xs[lo:hi], ys[lo:hi]))[0]) for _ in range(3)]}
    res['losses'].append(float(np.ravel(m.test_on_batch(xs[lo:hi], ys[lo:hi]))[0]))
    res['penalty_share'] = (res['losses'][0] - bare) / res['losses'][0]
    res['weights'] = m.get_weights()
    pickle.dump(res, open('%s.%d' % (out, rank), 'wb'))
    if dp:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
