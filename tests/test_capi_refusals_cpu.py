"""What the 47 streaming, optimizer, loss, BatchNorm, bias-gradient and weight-layout entry points answer before they touch the GPU: argument
refusals (code and gn_last_error text), the early GN_OK of an empty input, and the host-only workspace queries.  tests/golden/capi_refusals.json
was recorded (tests/tools/record_capi_refusals.py) from the library as it stood when capi.hip held a forwarding wrapper with the null checks
and each kernel file a launcher with the rest; an entry point is now one function beside its kernels and must still answer the same."""
import json
import os

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'capi_refusals.json')

ENTRY_POINTS = """
gn_act_fwd gn_act_bwd gn_act_dropout_bwd gn_dropout_mask gn_dropout_apply gn_upsample2_fwd gn_upsample2_bwd gn_subtract_stack_fwd
gn_subtract_stack_bwd gn_affine_stack_fwd gn_affine_stack_bwd gn_assemble_d_batch gn_gather_rows gn_axpy gn_fill_uniform gn_fill_normal
gn_fill_normal_dyn
gn_gaussian_noise_fwd gn_gaussian_dropout_apply gn_alpha_dropout_fwd gn_alpha_dropout_bwd
gn_optim_step gn_optim_sumsq_slots gn_optim_sumsq gn_optim_clip_factor gn_adam_step gn_adam_step_dyn
gn_bce_loss gn_mse_loss
gn_bn_stats_workspace gn_bn_stats gn_bn_finalize gn_bn_finalize_zero_debias gn_bn_finalize_zero_debias_dyn gn_bn_infer_coeffs gn_bn_apply
gn_bn_bwd_stats gn_bn_bwd_apply gn_bn_bwd_stats_conv1 gn_bn_bwd_apply_conv1 gn_bias_grad_workspace gn_bias_grad
gn_conv1d_transpose_w gn_conv2d_w2_fold gn_conv2d_w2_unfold_grad gn_conv1d_up2_fold gn_conv1d_up2_unfold_grad
""".split()


def test_fixture_covers_every_moved_entry_point_at_both_layers():
    from gennet_amd import _lib
    with open(FIXTURE) as f:
        cases = json.load(f)
    assert len(ENTRY_POINTS) == 47 and sorted(set(c['symbol'] for c in cases)) == sorted(ENTRY_POINTS)
    refused = set(c['symbol'] for c in cases if c['returns'] == _lib.GN_EINVAL and None in c['args'][:-1])
    queries = [s for s in ENTRY_POINTS if _lib.DECLS[s][0] is _lib.sz]
    assert refused == set(ENTRY_POINTS) - set(queries) and len(queries) == 3          # a null pointer for every function that takes one
    # the checks that used to sit in the launchers
    texts = set((c['symbol'], c['returns'], c['error']) for c in cases)
    for s in ('gn_upsample2_fwd', 'gn_upsample2_bwd'):
        assert (s, _lib.GN_EINVAL, 'upsample2: C 0 < 1') in texts
    for s in ('gn_bce_loss', 'gn_mse_loss'):
        assert (s, _lib.GN_EINVAL, 'loss: bad batch sizes 8 / 4') in texts
    assert ('gn_bias_grad', _lib.GN_EWORKSPACE, 'bias_grad: workspace too small') in texts
    assert ('gn_optim_step', _lib.GN_EINVAL, 'optim_step: unknown rule 99') in texts
    assert ('gn_optim_step', _lib.GN_EINVAL, 'optim_step: null pointer (rule 5 keeps 2 state arrays)') in texts
    assert ('gn_optim_step', _lib.GN_EINVAL, 'optim_step: beta_2 1.5 outside [0, 1]') in texts
    short_circuits = set(c['symbol'] for c in cases if c['returns'] == _lib.GN_OK and _lib.DECLS[c['symbol']][0] is _lib.i32)
    assert len(short_circuits) >= 25, sorted(short_circuits)


def test_entry_points_refuse_and_short_circuit_as_recorded():
    from gennet_amd import _lib
    L = _lib.lib()
    with open(FIXTURE) as f:
        cases = json.load(f)
    for c in cases:                         # in order: a GN_OK return leaves the text of the refusal before it
        returned = getattr(L, c['symbol'])(*c['args'])
        assert (int(returned), L.gn_last_error().decode()) == (c['returns'], c['error']), c
