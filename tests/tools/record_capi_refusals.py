"""Records tests/golden/capi_refusals.json: host-only calls of the streaming, optimizer, loss, BatchNorm, bias-gradient and weight-layout
entry points of libgennet_hip.so that return before any HIP call -- argument refusals, empty-input early returns, workspace queries -- each
as (symbol, arguments, return value, gn_last_error text after the call).  tests/test_capi_refusals_cpu.py replays the file in order.

    python tests/tools/record_capi_refusals.py          # rewrites the fixture from the library built in this tree

The fixture was recorded from the library as it stood BEFORE these entry points moved out of capi.hip to sit beside their kernels; run it
again only when an entry point's checks change on purpose.  A pointer argument is None (NULL) or P, an address nothing dereferences before
the refusal.  A call that returns GN_OK leaves the error text of the call before it, so the order of the cases is part of the record.
"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden', 'capi_refusals.json')

P = 4096
SGD, RMSPROP, ADAGRAD, ADAM, AMSGRAD = 0, 1, 2, 5, 6      # gn_optim_rule


def bn_finalize(sums=P, count=64.0, mm=P, mv=P):
    return [sums, count, P, P, 1e-3, 0.99, mm, mv, P, P, P, P, 8, None]


def bn_finalize_zd(step, sums=P):
    return [sums, 64.0, P, P, 1e-3, 0.99, P, P, P, P, step, P, P, P, P, 8, None]


def bn_bwd_stats(dy=P, y=P, scale=None, shift=None, ws_bytes=1 << 20, rows=64, C=8):
    return [dy, y, P, None, P, P, P, P, ws_bytes, rows, C, 0, 0.0, 0.0, scale, shift, None]


def bn_bwd_apply(dy=P, y=P, scale=None, shift=None, rows=64, C=8):
    return [dy, y, P, None, P, P, P, P, 64.0, P, P, P, P, rows, C, 0, 0.0, 0.0, scale, shift, None]


def bn_bwd_stats_conv1(g=P, L=16, k=5, x=P, ws_bytes=1 << 20, rows=64, C=8):
    return [g, P, L, L, k, 2, x, None, P, P, P, P, ws_bytes, rows, C, 0, 0.0, 0.0, P, P, None]


def bn_bwd_apply_conv1(g=P, L=16, k=5, x=P, rows=64, C=8):
    return [g, P, L, L, k, 2, x, None, P, P, P, P, 64.0, P, P, P, P, rows, C, 0, 0.0, 0.0, P, P, None]


def optim_step(rule, p=P, s1=P, s2=P, n=64, h0=0.9, h1=0.999, eps=1e-7):
    return [rule, p, P, P, s1, s2, n, 1e-3, None, h0, h1, eps, 0, None, 0.0, None]


CASES = [
    # ---- elementwise.hip
    ('gn_act_fwd', [None, P, 8, 1, 0.0, None]), ('gn_act_fwd', [P, P, 0, 1, 0.0, None]),
    ('gn_act_bwd', [P, None, P, 8, 1, 0.0, None]), ('gn_act_bwd', [P, P, P, 0, 1, 0.0, None]),
    ('gn_act_dropout_bwd', [P, P, None, P, 8, 1, 0.0, 0.5, None]), ('gn_act_dropout_bwd', [P, P, P, P, 8, 1, 0.0, 1.0, None]),
    ('gn_act_dropout_bwd', [P, P, P, P, 0, 1, 0.0, 0.5, None]),
    ('gn_dropout_mask', [None, 8, 0.5, 1, 0, None]), ('gn_dropout_mask', [P, 8, -0.25, 1, 0, None]), ('gn_dropout_mask', [P, 0, 0.5, 1, 0, None]),
    ('gn_dropout_apply', [P, None, P, 8, 0.5, None]), ('gn_dropout_apply', [P, P, P, 8, 1.0, None]), ('gn_dropout_apply', [P, P, P, 0, 0.5, None]),
    ('gn_upsample2_fwd', [None, P, 2, 8, 8, None]), ('gn_upsample2_fwd', [P, P, 2, 8, 0, None]), ('gn_upsample2_fwd', [P, P, 0, 8, 8, None]),
    ('gn_upsample2_bwd', [P, None, 2, 8, 8, None]), ('gn_upsample2_bwd', [P, P, 2, 8, 0, None]), ('gn_upsample2_bwd', [P, P, 2, 0, 8, None]),
    ('gn_subtract_stack_fwd', [P, None, P, 2, 8, None]), ('gn_subtract_stack_fwd', [P, P, P, 0, 8, None]),
    ('gn_subtract_stack_bwd', [None, P, 2, 8, None]), ('gn_subtract_stack_bwd', [P, P, 2, 0, None]),
    ('gn_affine_stack_fwd', [None, P, P, 1.0, -1.0, P, 2, 8, None]), ('gn_affine_stack_fwd', [P, None, None, 1.0, -1.0, P, 2, 0, None]),
    ('gn_affine_stack_fwd', [P, None, None, 1.0, -1.0, P, 0, 8, None]),
    ('gn_affine_stack_bwd', [P, 1.0, -1.0, None, 2, 8, None]), ('gn_affine_stack_bwd', [P, 1.0, -1.0, P, -1, 8, None]),
    ('gn_affine_stack_bwd', [P, 1.0, -1.0, P, 0, 8, None]),
    ('gn_assemble_d_batch', [P, P, None, P, P, 2, 8, None]), ('gn_assemble_d_batch', [P, P, P, P, P, 2, 0, None]),
    ('gn_assemble_d_batch', [P, P, P, P, P, 0, 8, None]),
    ('gn_gather_rows', [P, None, P, 4, 8, None]), ('gn_gather_rows', [P, P, P, 4, 0, None]), ('gn_gather_rows', [P, P, P, 0, 8, None]),
    ('gn_axpy', [None, P, 0.5, 8, None]), ('gn_axpy', [P, P, 0.5, 0, None]),
    ('gn_fill_uniform', [None, 8, 0.0, 1.0, 1, 0, None]), ('gn_fill_uniform', [P, 0, 0.0, 1.0, 1, 0, None]),
    ('gn_fill_normal', [None, 8, 0.0, 1.0, 1, 0, None]), ('gn_fill_normal', [P, 0, 0.0, 1.0, 1, 0, None]),
    ('gn_fill_normal_dyn', [P, 8, 0.0, None, 1, 0, None]), ('gn_fill_normal_dyn', [P, 0, 0.0, P, 1, 0, None]),
    # ---- noise_layers.hip
    ('gn_gaussian_noise_fwd', [None, P, 8, 0.1, 1, 0, None]), ('gn_gaussian_noise_fwd', [None, None, 0, 0.1, 1, 0, None]),
    ('gn_gaussian_dropout_apply', [P, None, 8, 0.1, 1, 0, None]), ('gn_gaussian_dropout_apply', [None, None, 0, 0.1, 1, 0, None]),
    ('gn_alpha_dropout_fwd', [None, P, 8, 0.1, 1.0, 0.0, -1.75, 1, 0, None]), ('gn_alpha_dropout_fwd', [P, P, 8, 0.0, 1.0, 0.0, -1.75, 1, 0, None]),
    ('gn_alpha_dropout_fwd', [None, None, 0, 0.1, 1.0, 0.0, -1.75, 1, 0, None]),
    ('gn_alpha_dropout_bwd', [P, None, 8, 0.1, 1.0, 1, 0, None]), ('gn_alpha_dropout_bwd', [P, P, 8, 1.0, 1.0, 1, 0, None]),
    ('gn_alpha_dropout_bwd', [None, None, 0, 0.1, 1.0, 1, 0, None]),
    # ---- optim.hip
    ('gn_optim_step', optim_step(99)), ('gn_optim_step', optim_step(-1)), ('gn_optim_step', optim_step(ADAM, p=None, n=0)),
    ('gn_optim_step', optim_step(SGD, p=None)), ('gn_optim_step', optim_step(ADAM, s1=None)), ('gn_optim_step', optim_step(AMSGRAD, s2=None)),
    ('gn_optim_step', optim_step(ADAM, eps=-1.0)), ('gn_optim_step', optim_step(RMSPROP, h0=1.5)), ('gn_optim_step', optim_step(ADAM, h1=1.5)),
    ('gn_optim_step', optim_step(ADAGRAD, s1=None, s2=None, n=0)),
    ('gn_optim_sumsq_slots', [0]), ('gn_optim_sumsq_slots', [1000]), ('gn_optim_sumsq_slots', [1023 * 1024]), ('gn_optim_sumsq_slots', [1 << 30]),
    ('gn_optim_sumsq', [P, 8, None, None]), ('gn_optim_sumsq', [None, 8, P, None]),
    ('gn_optim_clip_factor', [None, 4, 1.0, P, None]), ('gn_optim_clip_factor', [P, 0, 1.0, P, None]), ('gn_optim_clip_factor', [P, 4, 0.0, P, None]),
    ('gn_adam_step', [P, P, None, P, 8, 1e-3, 0.9, 0.999, 1e-7, None]), ('gn_adam_step', [P, P, P, P, 0, 1e-3, 0.9, 0.999, 1e-7, None]),
    ('gn_adam_step_dyn', [P, P, P, P, 8, None, 0.9, 0.999, 1e-7, None]), ('gn_adam_step_dyn', [P, P, P, P, 0, P, 0.9, 0.999, 1e-7, None]),
    # ---- loss.hip
    ('gn_bce_loss', [P, P, None, P, 8, 8, None]), ('gn_bce_loss', [P, P, P, P, 8, 4, None]), ('gn_bce_loss', [P, P, P, P, 0, 8, None]),
    ('gn_mse_loss', [None, P, P, P, 8, 8, None]), ('gn_mse_loss', [P, P, P, P, 8, 4, None]), ('gn_mse_loss', [P, P, P, P, 0, 8, None]),
    # ---- bn.hip
    ('gn_bn_stats_workspace', [1000, 64]), ('gn_bn_stats_workspace', [1000, 3]), ('gn_bn_stats_workspace', [7, 6]), ('gn_bn_stats_workspace', [1 << 20, 1024]),
    ('gn_bn_stats', [None, 64, 8, P, P, 1 << 20, None]), ('gn_bn_stats', [P, 0, 8, P, P, 1 << 20, None]), ('gn_bn_stats', [P, 64, 8, P, P, 16, None]),
    ('gn_bn_stats', [P, 64, 6, P, P, 16, None]),
    ('gn_bn_finalize', bn_finalize(sums=None)), ('gn_bn_finalize', bn_finalize(count=1.0)), ('gn_bn_finalize', bn_finalize(mv=None)),
    ('gn_bn_finalize_zero_debias', bn_finalize_zd(1, sums=None)), ('gn_bn_finalize_zero_debias', bn_finalize_zd(0)),
    ('gn_bn_finalize_zero_debias_dyn', bn_finalize_zd(P, sums=None)), ('gn_bn_finalize_zero_debias_dyn', bn_finalize_zd(None)),
    ('gn_bn_infer_coeffs', [P, P, None, P, 1e-3, P, P, 8, None]), ('gn_bn_infer_coeffs', [P, P, P, P, 1e-3, P, P, 0, None]),
    ('gn_bn_apply', [P, None, P, None, P, 64, 8, 0, 0.0, 0.0, None]), ('gn_bn_apply', [P, P, P, None, P, 64, 8, 0, 0.0, 0.5, None]),
    ('gn_bn_apply', [P, P, P, P, P, 64, 8, 0, 0.0, 1.0, None]), ('gn_bn_apply', [P, P, P, None, P, 0, 8, 0, 0.0, 0.0, None]),
    ('gn_bn_apply', [P, P, P, None, P, 0, 6, 0, 0.0, 0.0, None]),
    ('gn_bn_bwd_stats', bn_bwd_stats(dy=None)), ('gn_bn_bwd_stats', bn_bwd_stats(y=None)), ('gn_bn_bwd_stats', bn_bwd_stats(scale=P)),
    ('gn_bn_bwd_stats', bn_bwd_stats(rows=0)), ('gn_bn_bwd_stats', bn_bwd_stats(ws_bytes=16)),
    ('gn_bn_bwd_apply', bn_bwd_apply(dy=None)), ('gn_bn_bwd_apply', bn_bwd_apply(y=None)), ('gn_bn_bwd_apply', bn_bwd_apply(shift=P)),
    ('gn_bn_bwd_apply', bn_bwd_apply(rows=0)), ('gn_bn_bwd_apply', bn_bwd_apply(rows=0, C=6)),
    ('gn_bn_bwd_stats_conv1', bn_bwd_stats_conv1(x=None)), ('gn_bn_bwd_stats_conv1', bn_bwd_stats_conv1(g=None)),
    ('gn_bn_bwd_stats_conv1', bn_bwd_stats_conv1(C=6)), ('gn_bn_bwd_stats_conv1', bn_bwd_stats_conv1(rows=72)),
    ('gn_bn_bwd_stats_conv1', bn_bwd_stats_conv1(ws_bytes=16)),
    ('gn_bn_bwd_apply_conv1', bn_bwd_apply_conv1(x=None)), ('gn_bn_bwd_apply_conv1', bn_bwd_apply_conv1(k=6)),
    ('gn_bn_bwd_apply_conv1', bn_bwd_apply_conv1(C=6)), ('gn_bn_bwd_apply_conv1', bn_bwd_apply_conv1(rows=72)),
    ('gn_bn_bwd_apply_conv1', bn_bwd_apply_conv1(rows=0)),
    ('gn_bias_grad_workspace', [1000, 64]), ('gn_bias_grad_workspace', [1000, 3]), ('gn_bias_grad_workspace', [10, 6]),
    ('gn_bias_grad', [P, None, P, 1 << 20, 64, 8, None]), ('gn_bias_grad', [P, P, P, 1 << 20, 0, 8, None]), ('gn_bias_grad', [P, P, P, 16, 64, 3, None]),
    ('gn_bias_grad', [P, P, P, 16, 64, 8, None]), ('gn_bias_grad', [P, P, P, 16, 64, 6, None]),
    # ---- weight_layout.hip
    ('gn_conv1d_transpose_w', [P, None, 5, 8, 8, None]), ('gn_conv1d_transpose_w', [P, P, 0, 8, 8, None]),
    ('gn_conv2d_w2_fold', [None, P, P, P, 3, 8, 8, None]), ('gn_conv2d_w2_fold', [P, None, P, None, 0, 8, 8, None]),
    ('gn_conv2d_w2_unfold_grad', [P, P, None, P, 3, 8, 8, None]), ('gn_conv2d_w2_unfold_grad', [P, P, P, P, 3, 0, 8, None]),
    ('gn_conv1d_up2_fold', [P, P, None, P, 8, 8, 1, None]), ('gn_conv1d_up2_fold', [P, P, P, P, 8, 8, 3, None]),
    ('gn_conv1d_up2_unfold_grad', [None, P, P, P, 8, 8, 2, None]), ('gn_conv1d_up2_unfold_grad', [P, None, P, P, 8, 8, 2, None]),
]


def main():
    from gennet_amd import _lib
    L = _lib.lib()
    records = []
    for symbol, args in CASES:
        returned = getattr(L, symbol)(*args)
        records.append({'symbol': symbol, 'args': args, 'returns': int(returned), 'error': L.gn_last_error().decode()})
    with open(OUT, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(r) for r in records) + '\n]\n')
    print('%d cases of %d entry points -> %s' % (len(records), len(set(s for s, _ in CASES)), os.path.relpath(OUT, ROOT)))


if __name__ == '__main__':
    main()
