"""Pins tests/refs64_nonfinite.py (CPU only): the poisoned references against torch's own modules on doubles (F.linear / F.conv2d / autograd /
F.max_pool2d with torch's activations: the same NaN and +-inf pattern, the finite part to 1e-12); that the SAME reference in float32 gives the
same pattern as float64 on every case, the precondition of an exact pattern check on the device; that every named mistake changes the pattern
of at least one element on every case it applies to; that every activation and loss kind is poisoned by some case and every row of
DENSE_CASES and CONV_CASES has a poisoned case; that the activation variants of tests/test_nonfinite_kernels_gpu.py stay on their kernel."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import refs64_conv as C
import refs64_gemm as G
import refs64_nonfinite as R

f32, f64 = torch.float32, torch.float64


def _lib():
    from robust_e2e_gan_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return lib


@functools.lru_cache(maxsize=None)
def _dense(i):
    row = G.DENSE_CASES[i]
    clean = G.dense_case(row)
    case = R.poison_dense(row, clean)
    return row, clean, case, R.dense_expected(row, case, clean), R.dense_expected(row, case, clean, f32)


@functools.lru_cache(maxsize=None)
def _conv(i):
    row = C.CONV_CASES[i]
    case = R.poison_conv(row, C.conv_case(row))
    return row, case, R.conv_expected(row, case), R.conv_expected(row, case, f32)


def _values(out):
    return out[0] if isinstance(out, tuple) else out


DENSE_IDS = [G.case_id(r) for r in G.DENSE_CASES]
CONV_IDS = [C.case_id(r) for r in C.CONV_CASES]
_TORCH_ACT = {R.ACT_NONE: lambda t: t, R.ACT_TANH: torch.tanh, R.ACT_RELU: torch.relu, R.ACT_LRELU: lambda t: F.leaky_relu(t, 0.2), R.ACT_SIGMOID: torch.sigmoid}


def _equal_to_torch(got, want, tag):
    assert R.same_pattern(got, want), (tag, 'the non-finite pattern differs from torch\'s')
    assert R.finite_err(got, want) <= 1e-12, (tag, R.finite_err(got, want))


# ---------------------------------------------------------------------------------------------
# pinning
# ---------------------------------------------------------------------------------------------
def test_activations_of_the_sibling_references_follow_torch():
    """clamp(min=0) and where(v > 0, v, 0.2 v), what refs64_gemm._act / refs64_conv._act write, ARE relu / leaky_relu on NaN and +-inf; and
    fmax(v, 0.2 v) is leaky_relu too (the 'mistake' that is none)."""
    v = torch.tensor(R.SPECIALS + (3e38, -3e38, 1e-45, -1e-45), dtype=f64)
    for dt in (f64, f32):
        x = v.to(dt)
        for act, fn in _TORCH_ACT.items():
            assert R.same_pattern(G._act(x, act), fn(x)) and R.finite_err(G._act(x, act), fn(x)) == 0
            assert R.same_pattern(R.act_ref(x, act), fn(x)) and R.finite_err(R.act_ref(x, act), fn(x)) == 0
        for act in (C.ACT_NONE, C.ACT_RELU, C.ACT_LRELU):
            assert R.same_pattern(C._act(x, act), _TORCH_ACT[act](x))
        lr = R.act_ref(x, R.ACT_LRELU, 'leaky relu by max(v, 0.2 v)')
        assert R.same_pattern(lr, F.leaky_relu(x, 0.2)) and R.finite_err(lr, F.leaky_relu(x, 0.2)) == 0
        assert R.same_pattern(torch.maximum(x, 0.2 * x), F.leaky_relu(x, 0.2))
    assert torch.isnan(torch.relu(torch.tensor(R.NAN))) and torch.relu(torch.tensor(-R.INF)) == 0 and torch.relu(torch.tensor(R.INF)) == R.INF


@pytest.mark.parametrize('i', [i for i, r in enumerate(G.DENSE_CASES) if r.M * r.N * r.K <= 1 << 24], ids=lambda i: DENSE_IDS[i])
def test_dense_reference_is_linear_plus_activation_on_poisoned_inputs(i):
    row, clean, case, e64, _ = _dense(i)
    A, B = case['A'].double(), case['B'].double()
    m = case['map']
    if row.op == 'nt':
        pre = F.linear(A[m] if row.entry == 'nt_rows' else A, B)
    elif row.op == 'nn':
        pre = A @ B
    else:
        pre = (A[m].t() @ B[m]) if row.entry == 'tn_rows' else A.t() @ B
    if row.bias:
        pre = pre + case['b1'].double()
    if row.bias2:
        pre = pre + case['b2'].double()
    c0 = case['C0'].double()
    c0 = c0[m] if row.entry == 'nt_rows' else c0
    if row.act == R.ACT_MASK:
        live = (torch.arange(row.M) % row.T) < case['lens'][torch.arange(row.M) // row.T]
        mask = torch.where(live[:, None], torch.sigmoid(pre), torch.zeros_like(pre))
        _equal_to_torch(e64['mask_out'], mask, 'mask_out')
        want = mask * case['mul'].double()
        assert (want[~live] == 0).all() and not live[[r for k, r, _ in case['poison'] if k in ('+inf', 'nan_beyond')]].any()
    else:
        want = _TORCH_ACT[row.act](pre) + row.beta * c0
    assert e64['rows'] == list(range(row.M))
    _equal_to_torch(e64['C'], want, DENSE_IDS[i])
    bad = ~torch.isfinite(e64['C'])
    assert bad.any() and not bad[[r for r in range(row.M) if r not in {p[1] for p in case['poison']}]].any(), 'only the poisoned rows are non-finite'


@pytest.mark.parametrize('i', [i for i, r in enumerate(C.CONV_CASES) if r.N * r.H * r.W * r.Cin * r.Cout <= 1 << 21], ids=lambda i: CONV_IDS[i])
def test_conv_reference_is_conv2d_plus_activation_on_poisoned_inputs(i):
    row, case, e64, _ = _conv(i)
    x = case['x'].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    w = case['w'].double().clone().requires_grad_(True)
    b = case['b'].double() if row.flags & C.F_BIAS else None
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    if row.direction == C.FWD:
        y = _TORCH_ACT[row.act](F.conv2d(x, w, b, row.stride, row.pad))
        if row.beta:
            y = y + case['y0'].double().permute(0, 3, 1, 2)
        if row.flags & C.F_POOL:
            y = F.max_pool2d(y, 2, 2, ceil_mode=True)
        _equal_to_torch(_values(e64), nhwc(y.detach()), CONV_IDS[i])
        return
    go = case['dz'].double().permute(0, 3, 1, 2)
    if row.direction == C.DGRAD:
        xin = x
        if row.flags & C.F_MASK:          # x is the ReLU output of the layer in front: the gradient goes through threshold_backward
            pre = case['x'].double().permute(0, 3, 1, 2).clone()
            pre[pre == 0] = -1.0
            xin = pre.requires_grad_(True)
            (dx,) = torch.autograd.grad(F.conv2d(torch.relu(xin), w, None, row.stride, row.pad), xin, go)
        else:
            (dx,) = torch.autograd.grad(F.conv2d(xin, w, None, row.stride, row.pad), xin, go)
        _equal_to_torch(e64, nhwc(dx), CONV_IDS[i])
    else:
        (dw,) = torch.autograd.grad(F.conv2d(x, w, None, row.stride, row.pad), w, go)
        _equal_to_torch(e64, dw + (case['dW0'].double() if row.beta else 0), CONV_IDS[i])


def test_pointwise_references_are_autograd_and_torchs_losses():
    for M, N in ((24, 16), (37, 10)):
        dy, y = R.act_bwd_table(M, N)
        for act, inv in ((R.ACT_TANH, torch.atanh), (R.ACT_SIGMOID, torch.logit), (R.ACT_RELU, None), (R.ACT_LRELU, None)):
            ys = y * 0.5 + 0.5 if act == R.ACT_SIGMOID else y          # (a sigmoid's output lies in (0, 1); the kernel's formula takes any y)
            yd = ys.double()
            x =(inv(yd) if inv else torch.where(yd > 0, yd, yd - 1.0 if act == R.ACT_RELU else yd * 5 - 1e-3)).requires_grad_(True)
            out = _TORCH_ACT[act](x)
            (want,) = torch.autograd.grad(out, x, dy.double())
            dz, cs = R.act_bwd_ref(dy, ys, act)
            assert R.same_pattern(dz, want) and R.finite_err(dz, want) <= 1e-9, act
            assert R.same_pattern(cs, want.sum(0))
            assert torch.isnan(cs[0]) and cs[1] == R.INF and cs[2] == -R.INF and torch.isnan(cs[3]) and torch.isnan(cs[-1]) and torch.isfinite(cs[4:-1]).all()
    # BCE: ATen's formula written out is F.binary_cross_entropy wherever that accepts the input, autograd included
    a, t = R.loss_table(R.BCE, 'finite')
    val, grad = R.loss_ref(R.BCE, a, t)
    x = a.double().requires_grad_(True)
    want = F.binary_cross_entropy(x, t.double())
    want.backward()
    assert abs(val.item() - want.item()) <= 1e-12 * want.item() and R.finite_err(grad, x.grad) <= 1e-12 and torch.isfinite(grad).all()
    with pytest.raises(RuntimeError):
        F.binary_cross_entropy(torch.tensor([R.NAN], dtype=f64), torch.tensor([0.3], dtype=f64))
    terms, _ = R.bce_ref(torch.tensor([0.0, 1.0, 0.0, 1.0]), torch.tensor([1.0, 0.0, 0.25, 0.25]))
    assert terms.tolist() == [100.0, 100.0, 25.0, 75.0], 'the -100 clamp holds at a = 0 and a = 1'


# ---------------------------------------------------------------------------------------------
# float32 gives the pattern of float64; the mistakes change it; nothing is left out
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(G.DENSE_CASES)), ids=lambda i: DENSE_IDS[i])
def test_dense_pattern_in_float32_and_under_every_mistake(i):
    row, clean, case, e64, e32 = _dense(i)
    for k in ('C', 'mask_out'):
        if k in e64:
            assert R.same_pattern(e32[k], e64[k]), 'float32 alone moves the pattern: change the input'
            assert R.finite_err(e32[k], e64[k], e64['scale']) <= G.BARS[G.family_of(row, row.plan)][0] / 8
    assert not torch.isfinite(e64['C']).all()
    for mk in R.dense_mistakes_of(row):
        wrong = R.dense_expected(row, case, clean, mistake=mk)
        assert any(not R.same_pattern(wrong[k], e64[k]) for k in ('C', 'mask_out') if k in e64), ('the case is blind to', mk)


@pytest.mark.parametrize('i', range(len(C.CONV_CASES)), ids=lambda i: CONV_IDS[i])
def test_conv_pattern_in_float32_and_under_every_mistake(i):
    row, case, e64, e32 = _conv(i)
    assert R.same_pattern(_values(e32), _values(e64)), 'float32 alone moves the pattern: change the input'
    assert not torch.isfinite(_values(e64)).all()
    for mk in R.conv_mistakes_of(row, case):
        wrong = R.conv_expected(row, case, mistake=mk)
        assert not R.same_pattern(_values(wrong), _values(e64)), ('the case is blind to', mk)
    if C.family_of(row) != 'direct':          # every non-finite element of the reference lies in a tile a Winograd kernel may spoil
        assert R.touched(row, case)[~torch.isfinite(_values(e64))].all() and (row.H * row.W <= 64 or not R.touched(row, case).all())


def test_pointwise_patterns_in_float32_and_under_the_log_clamp_mistake():
    for kind in (R.L2, R.L1, R.SMOOTH_L1, R.BCE):
        for poison in ('finite', 'nan') + (('inf',) if kind != R.BCE else ()):
            a, t = R.loss_table(kind, poison)
            v64, g64 = R.loss_ref(kind, a, t)
            v32, g32 = R.loss_ref(kind, a, t, f32)
            assert R.same_pattern(v32, v64) and R.same_pattern(g32, g64), (kind, poison)
            assert torch.isnan(v64) == (poison == 'nan') and torch.isfinite(v64) == (poison == 'finite')
            if poison == 'nan':
                nan_in = torch.isnan(a)
                assert nan_in.any() and (torch.isnan(g64[nan_in]).all() if kind != R.L1 else (g64[nan_in] == 0).all()), 'torch: sign(NaN) = 0'
    a, t = R.loss_table(R.BCE, 'nan')
    wrong, _ = R.loss_ref(R.BCE, a, t, mistake='log clamp by fmax')
    assert torch.isfinite(wrong) and torch.isnan(R.loss_ref(R.BCE, a, t)[0])
    for n in (5, 4099 + 13):
        x = R.act_table(n)
        for act in R.ACTS:
            assert R.same_pattern(R.act_ref(x, act), R.act_ref(x.double(), act)) and torch.isnan(R.act_ref(x, act)[-1])
    x = R.act_table(5)
    assert not R.same_pattern(R.act_ref(x, R.ACT_RELU, 'relu by fmax'), torch.relu(x)) and not R.same_pattern(R.act_ref(x, R.ACT_RELU, 'relu as max(v, 0 v)'), torch.relu(x))


def test_nothing_is_left_out():
    missing = []
    for row in G.DENSE_CASES:
        try:
            case = R.poison_dense(row, G.dense_case(row))
            kinds = {p[0] for p in case['poison']}
            assert {'nan', '+inf', '-inf', 'nan_last'} <= kinds and max(p[1] for p in case['poison']) == row.M - 1
        except AssertionError:
            missing.append(G.case_id(row))
    for row in C.CONV_CASES:
        try:
            case = R.poison_conv(row, C.conv_case(row))
            assert {'nan', 'nan_last'} <= {p[0] for p in case['poison']}
        except AssertionError:
            missing.append(C.case_id(row))
    assert missing == []
    acts = {row.act for row in G.DENSE_CASES} | {row.act for _, row in R.dense_variants()}
    assert acts == set(range(6)), 'every activation, the mask epilogue included, meets a poisoned case'
    assert {row.act for row in C.CONV_CASES if row.direction == C.FWD} >= {C.ACT_NONE, C.ACT_RELU}
    assert {r.act for _, r in R.conv_variants()} == {C.ACT_RELU, C.ACT_LRELU}          # (every site's smallest row is one without an activation)
    used = {m for row in G.DENSE_CASES for m in R.dense_mistakes_of(row)} | \
        {m for row in C.CONV_CASES for m in R.conv_mistakes_of(row, R.poison_conv(row, C.conv_case(row)))} | {'log clamp by fmax'}
    assert used == set(R.MISTAKES) - {'leaky relu by max(v, 0.2 v)'}
    # +inf and -inf, too, wherever the geometry leaves room: more than half of the convolution rows, every family among them
    full = [row for row in C.CONV_CASES if {'+inf', '-inf'} <= {p[0] for p in R.poison_conv(row, C.conv_case(row))['poison']}]
    assert len(full) > len(C.CONV_CASES) // 2 and {C.family_of(r) for r in full} == {'direct', 'wino3x3', 'wino4x4'}
    assert {r.direction for r in full} == {C.FWD, C.DGRAD, C.WGRAD}


def test_activation_variants_stay_on_their_kernel():
    lib = _lib()
    sites = {s for s, _ in R.dense_variants()}
    assert sites == {'engine one slice', 'engine beta = 1', 'engine split', 'engine zx', 'pipeline dp', 'pipeline dp+sk', 'pipeline sk'}
    for site, row in R.dense_variants():
        args, kw = G.plan_args(row)
        assert G.form_key(lib.gemm_plan(*args, cus=256, **kw), row) == row.form, (site, G.case_id(row))
    assert {s for s, _ in R.conv_variants()} == {'cin1_fwd', 'cout1 generic', 'cout1 fixed taps', 'cout1_rows', 'halo', 'engine', 'pipeline', 'wino3x3'}
    for site, row in R.conv_variants():
        args, flags = C.plan_args(row)
        assert R.same_site(row.form, C.form_key(row.direction, lib.conv_plan(*args, flags=flags, cus=256))), (site, C.case_id(row))
