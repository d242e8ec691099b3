"""Pins tests/refs64_conv.py (CPU only): the float64 layer reference against F.conv2d, F.conv_transpose2d, autograd and
F.max_pool2d(ceil_mode=True) on doubles, and the Winograd evaluations against it; that ``CONV_CASES`` names exactly the kernel forms the
convolution plans (re2e_conv_plan) can name on a 256-CU chip, every row with the plan and the sub-form it declares; that the bars of
tests/test_conv_kernels_gpu.py are what their rule gives (8 x the worst distance of the fp32 CPU yardstick from float64 over every input of that
test, rounded up to one significant digit, none above 5e-5); and that every input can SEE a wrong kernel (seven deliberate mistakes in the
reference, each on every row it applies to).

The closure sweep below names 93 forms under refs64_conv.form_key; CONV_CASES holds 118 rows (25 more for the Winograd sub-forms), and
NEVER_NAMED the two built forms no plan reaches."""
import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

import refs64_conv as R

ALL = list(R.CONV_CASES) + list(R.EDGES)


def _lib():
    from robust_e2e_gan_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return lib


def _plan(row):
    args, flags = R.plan_args(row)
    return _lib().conv_plan(*args, flags=flags, cus=256)


@functools.lru_cache(maxsize=None)
def _measured(row):
    """-> (family, quantity, float64 reference, distance of the fp32 yardstick from it)."""
    fam = R.family_of(row, None if row.form is not None or row.via else _plan(row)['family'])
    case = R.conv_case(row)
    ref = R.case_ref(row, case)
    ref = ref[0] if row.flags & R.F_POOL else ref
    return fam, R.quantity_of(row), ref, R.rel_err(R.case_yardstick(row, case, fam), ref)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


# ---------------------------------------------------------------------------------------------
# pinning
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,H,W,Cin,Cout,k,s,p', [(2, 7, 5, 3, 4, 3, 1, 1), (1, 9, 11, 5, 2, 4, 1, 1), (2, 8, 6, 3, 5, 4, 2, 1), (1, 1, 9, 4, 3, 3, 1, 1),
                                                   (2, 6, 1, 2, 3, 3, 1, 1), (1, 10, 2, 1, 6, 4, 2, 1), (1, 5, 7, 6, 1, 3, 1, 0)])
def test_layer_reference_is_conv2d_and_its_autograd_in_double(N, H, W, Cin, Cout, k, s, p):
    g = torch.Generator().manual_seed(H * 100 + W)
    x, w, b = [R.rnd(g, *sh).double() for sh in ((N, H, W, Cin), (Cout, Cin, k, k), (Cout,))]
    for act, fn in ((R.ACT_NONE, lambda t: t), (R.ACT_RELU, F.relu), (R.ACT_LRELU, lambda t: F.leaky_relu(t, 0.2))):
        want = _nhwc(fn(F.conv2d(_nchw(x), w, b, stride=s, padding=p)))
        assert R.rel_err(R.conv_fwd(x, w, b, s, p, act), want) <= 1e-12
    y0 = R.rnd(g, *want.shape).double()
    want = _nhwc(F.relu(F.conv2d(_nchw(x), w, b, stride=s, padding=p)))
    assert R.rel_err(R.conv_fwd(x, w, b, s, p, R.ACT_RELU, y0), want + y0) <= 1e-12          # beta = 1: added behind the activation
    xr, wr, br = [t.clone().requires_grad_(True) for t in (x, w, b)]
    yr = _nhwc(F.conv2d(_nchw(xr), wr, br, stride=s, padding=p))
    dz = R.rnd(g, *yr.shape).double()
    (yr * dz).sum().backward()
    assert R.rel_err(R.conv_dgrad(dz, w, H, W, s, p), xr.grad) <= 1e-12
    assert R.rel_err(R.conv_wgrad(x, dz, k, k, s, p), wr.grad) <= 1e-12
    dW0 = R.rnd(g, *w.shape).double()
    assert R.rel_err(R.conv_wgrad(x, dz, k, k, s, p, dW0), wr.grad + dW0) <= 1e-12
    assert R.rel_err(R.bias_grad(dz), br.grad) <= 1e-12
    if s == 1:      # through the ReLU of the layer in front: its OUTPUT is the mask, exact zeros block
        pre = R.rnd(g, N, H, W, Cin).double().requires_grad_(True)
        relu_out = F.relu(pre)
        (_nhwc(F.conv2d(_nchw(relu_out), w, None, stride=1, padding=p)) * dz).sum().backward()
        got = R.conv_dgrad(dz, w, H, W, 1, p, relu_out.detach())
        assert R.rel_err(got, pre.grad) <= 1e-12 and (got[relu_out.detach() == 0] == 0).all() and (relu_out == 0).any()


@pytest.mark.parametrize('N,H,W,C1,C2', [(2, 5, 3, 3, 4), (1, 1, 6, 2, 5), (1, 4, 1, 4, 1)])
def test_transposed_reference_is_conv_transpose2d_in_double(N, H, W, C1, C2):
    g = torch.Generator().manual_seed(H * 100 + W)
    x, wt, b = [R.rnd(g, *sh).double().requires_grad_(True) for sh in ((N, H, W, C1), (C1, C2, 4, 4), (C2,))]
    yr = _nhwc(F.conv_transpose2d(_nchw(x), wt, b, stride=2, padding=1))
    dy = R.rnd(g, *yr.shape).double()
    (yr * dy).sum().backward()
    assert yr.shape == (N, 2 * H, 2 * W, C2)
    assert R.rel_err(R.conv_transpose_fwd(x.detach(), wt.detach(), b.detach()), yr) <= 1e-12
    dx, dwt, db = R.conv_transpose_grads(x.detach(), wt.detach(), dy)
    assert R.rel_err(dx, x.grad) <= 1e-12 and R.rel_err(dwt, wt.grad) <= 1e-12 and R.rel_err(db, b.grad) <= 1e-12


@pytest.mark.parametrize('N,H,W,C', [(2, 7, 5, 3), (1, 1, 6, 2), (1, 6, 1, 4), (2, 4, 4, 1), (1, 1, 1, 3)])
def test_pool_reference_is_max_pool2d_ceil_mode_with_first_maximum_indices(N, H, W, C):
    """On a ReLU output quantised to halves: ties inside most windows, all-zero windows common."""
    g = torch.Generator().manual_seed(H * 100 + W)
    y = F.relu(torch.round(R.rnd(g, N, H, W, C) * 2) / 2).double()
    vals, idx = R.relu_pool(y)
    want, flat = F.max_pool2d(_nchw(y), 2, stride=2, ceil_mode=True, return_indices=True)
    assert torch.equal(vals, _nhwc(want))
    flat = _nhwc(flat)
    pos = (flat // W % 2) * 2 + flat % W % 2          # torch's index into the H x W plane -> dy * 2 + dx of its window
    live = vals > 0
    assert torch.equal(idx[live].long(), pos[live]) and (idx[~live] == 4).all() and (~live).any()
    # ties: the first maximum in row-major order
    assert torch.equal(R.relu_pool(torch.ones(1, 2, 2, 1).double())[1], torch.zeros(1, 1, 1, 1, dtype=torch.uint8))
    t = torch.tensor([0., 3., 3., 3.]).view(1, 2, 2, 1).double()
    assert R.relu_pool(t)[1].item() == 1


@pytest.mark.parametrize('r,pad,H,W', [(3, 1, 7, 6), (3, 1, 1, 2), (4, 1, 7, 6), (4, 2, 6, 7), (4, 1, 2, 5)])
def test_winograd_evaluations_are_the_direct_convolution_in_double(r, pad, H, W):
    g = torch.Generator().manual_seed(H * 100 + W + r)
    x, w = R.rnd(g, 2, H, W, 5).double(), R.rnd(g, 3, 5, r, r).double()
    ref = R.conv_fwd(x, w, None, 1, pad)
    assert R.rel_err(R.wino_fwd(x, w, pad, torch.float64), ref) <= 1e-12
    dz = R.rnd(g, *ref.shape).double()
    assert R.rel_err(R.wino_dgrad(dz, w, pad, torch.float64), R.conv_dgrad(dz, w, H, W, 1, pad)) <= 1e-12
    assert R.rel_err(R.wino_wgrad(x, dz, r, pad, torch.float64), R.conv_wgrad(x, dz, r, r, 1, pad)) <= 1e-12


@pytest.mark.parametrize('layer', R.LAYERS, ids=R.layer_id)
def test_layer_gradients_are_autograd_in_double(layer):
    N, H, W, Cin, Cout, k, stride, act, bias, transposed = layer
    case = R.layer_case(layer)
    leaves = {n: case[n].double().requires_grad_(True) for n in ('x', 'w', 'b') if case[n] is not None}
    if transposed:
        y = _nhwc(F.conv_transpose2d(_nchw(leaves['x']), leaves['w'], leaves.get('b'), stride=2, padding=1))
    else:
        y = _nhwc(F.conv2d(_nchw(leaves['x']), leaves['w'], leaves.get('b'), stride=stride, padding=1))
        y = {R.ACT_NONE: lambda t: t, R.ACT_RELU: F.relu, R.ACT_LRELU: lambda t: F.leaky_relu(t, 0.2)}[act](y)
    (y * case['go'].double()).sum().backward()
    r64, r32 = R.layer_ref(layer, case), R.layer_ref(layer, case, torch.float32)
    for name, leaf in (('y', None), ('dx', 'x'), ('dW', 'w'), ('db', 'b')):
        if r64[name] is None:
            continue
        assert R.rel_err(r64[name], y if leaf is None else leaves[leaf].grad) <= 1e-12, name
        e = R.rel_err(r32[name], r64[name])
        print('MARGIN %-40s %-3s fp32-cpu %.2e' % (R.layer_id(layer), name, e))
        assert e <= R.BARS[name, 'direct'] / 8, name          # (every Winograd bar is at or above the direct one)


# ---------------------------------------------------------------------------------------------
# closure
# ---------------------------------------------------------------------------------------------
_SIZES = ((1, 5, 3), (1, 9, 8), (2, 33, 8), (1, 35, 19), (3, 21, 24), (1, 17, 250), (1, 66, 66), (2, 64, 64), (8, 64, 40), (16, 64, 64), (32, 100, 40), (128, 800, 80))
_CIN = (1, 3, 4, 6, 8, 12, 16, 20, 32, 36, 64, 96, 128, 192, 256, 512, 1024)
_COUT = (1, 2, 4, 6, 8, 10, 12, 16, 20, 32, 36, 64, 96, 100, 128, 192, 256, 512)


def _sweep():
    """3x3 / stride 1, 4x4 / stride 1 and 4x4 / stride 2 (pad 1) over 12 image sizes and 17 x 18 channel pairs, in every direction, with and
    without the Winograd families, through a ReLU mask, with the fused pool, with no activation and with ReLU, aligned and not, on the main and
    on a filler stream."""
    for k, s in ((3, 1), (4, 1), (4, 2)):
        for N, H, W in _SIZES:
            if s == 2:
                H, W = H + H % 2, W + W % 2
            for Cin in _CIN:
                for Cout in _COUT:
                    for d in (R.FWD, R.DGRAD, R.WGRAD):
                        extras = [0, R.F_DIRECT]
                        if d == R.DGRAD and s == 1:
                            extras += [R.F_MASK, R.F_MASK | R.F_NO_WINO]
                        if d == R.FWD and k == 3:
                            extras += [R.F_POOL | R.F_BIAS, R.F_POOL | R.F_BIAS | R.F_NO_WINO]
                        for e in extras:
                            for act in ((R.ACT_RELU,) if e & R.F_POOL else (R.ACT_NONE, R.ACT_RELU) if d == R.FWD else (R.ACT_NONE,)):
                                for u in (0, R.F_UNALIGNED):
                                    for f in (0, R.F_FILLER):
                                        yield (d, N, H, W, Cin, Cout, k, k, s, 1, 0, 0, act), e | u | f


def test_cases_are_closed_under_the_plans():
    """No device is touched (cus = 256).  Every form a plan names over the sweep has a row in CONV_CASES and the other way round; what is built
    and never named is NEVER_NAMED; every row's declared plan is what the library answers, every Winograd row's sub-form what the launch
    arithmetic gives -- checked against the workspace sizes the library itself answers, which are functions of that arithmetic."""
    lib = _lib()
    named, points = set(), 0
    for args, flags in _sweep():
        points += 1
        named.add(R.form_key(args[0], lib.conv_plan(*args, flags=flags, cus=256)))
    assert points == 440640
    declared = {row.form for row in R.CONV_CASES}
    assert named == declared, ('reachable without a numeric case', sorted(named - declared, key=str), 'declared and never named', sorted(declared - named, key=str))
    assert len(named) == 93
    for row in ALL:
        got = R.form_key(row.direction, _plan(row))
        assert row.form is None or got == row.form, (R.case_id(row), got)
        assert got not in R.NEVER_NAMED
        if row.form is not None:
            assert R.sub_of(row) == row.sub, (R.case_id(row), R.sub_of(row))
    assert not set(R.NEVER_NAMED) & named
    ids = [R.case_id(row) for row in ALL]
    assert len(set(ids)) == len(ids)
    # every sub-form the issue of the Winograd files asks for has a row
    subs = {(row.form, row.sub) for row in R.CONV_CASES}
    for shape in ('wide', 'tall'):
        for staging in ('c64', 'passes', 'lanes'):
            for groups in (1, 2, 4):
                assert (('wino3x3', R.FWD), (shape, staging, groups)) in subs
        assert any(f == ('wino3x3', R.WGRAD) and s[0] == shape for f, s in subs)
    nsplits = {s[1] for f, s in subs if f == ('wino3x3', R.WGRAD)}
    assert 1 in nsplits and any(n % 8 and n > 1 for n in nsplits) and any(n >= 8 for n in nsplits)
    assert {s for f, s in subs if f == ('wino4x4', R.WGRAD)} == {('sub', 1, 'exact'), ('sub', 2, 'padded')}
    so = lib.load()
    for row in ALL:
        fam = R.family_of(row, _plan(row)['family'])
        if row.direction == R.WGRAD and fam == 'wino3x3':
            assert so.re2e_conv3x3_wino_wgrad_workspace_bytes(row.N, row.H, row.W, row.Cin, row.Cout) == R.ww_workspace_bytes(row.N, row.H, row.W, row.Cin, row.Cout)
        if row.direction == R.WGRAD and fam == 'wino4x4':
            assert so.re2e_conv4x4_wino_wgrad_workspace_bytes(row.N, row.H, row.W, row.Cin, row.Cout, row.pad) == \
                R.w44_wgrad_sub(row.N, row.H, row.W, row.Cin, row.Cout, row.pad)[3]


def test_cout1_rows_is_planned_only_while_its_table_fits_the_lds():
    """The row-tile Cout == 1 kernel keeps an [18][W + 2][9] float table in LDS: 163 296 bytes at W = 250, 163 944 at W = 251, a CU has 163 840."""
    lib = _lib()
    for d, cin, cout in ((R.FWD, 64, 1), (R.DGRAD, 1, 64)):
        for W in range(16, 300):
            p = lib.conv_plan(d, 1, 20, W, cin, cout, 3, 3, 1, 1, cus=256)
            if W <= 250:
                assert p['route'] == 'cout1_rows' and int(p['lds']) == 18 * (W + 2) * 9 * 4 <= 160 * 1024, (W, p)
            else:
                assert (p['route'], p['L'], p['kh'], p['kw'], p['ch']) == ('cout1', '16', '3', '3', '1') and int(p['lds']) <= 64 * 1024, (W, p)
    # the Cin == 1 weight gradient stages KH rows of the image: rows too long for the 64 KiB a plain launch may ask for go to the engine
    assert lib.conv_plan(R.WGRAD, 1, 4, 4000, 1, 64, 3, 3, 1, 1, cus=256)['route'] == 'wgrad_cin1'
    assert lib.conv_plan(R.WGRAD, 1, 4, 6000, 1, 64, 3, 3, 1, 1, cus=256)['route'] == 'wgrad_engine'
    assert lib.conv_plan(R.WGRAD, 1, 4, 6000, 1, 64, 4, 4, 2, 1, cus=256)['route'] == 'wgrad_engine'


# ---------------------------------------------------------------------------------------------
# bars and sensitivity
# ---------------------------------------------------------------------------------------------
def _round_up_one_digit(v):
    e = math.floor(math.log10(v))
    return math.ceil(v / 10 ** e - 1e-9) * 10 ** e


def test_bars_are_eight_times_the_worst_fp32_yardstick():
    worst = {}
    for row in ALL:
        fam, q, _, e = _measured(row)
        print('MARGIN %-78s %-4s %-7s fp32-cpu %.2e  bar %.0e' % (R.case_id(row), q, fam, e, R.BARS[q, fam]))
        assert e <= R.BARS[q, fam] / 8, (R.case_id(row), e)
        worst[q, fam] = max(worst.get((q, fam), 0.0), e)
    for layer in R.LAYERS:          # whole layers: the direct reference in float32 (the yardstick of the direct family; db has no other)
        case = R.layer_case(layer)
        r64, r32 = R.layer_ref(layer, case), R.layer_ref(layer, case, torch.float32)
        for q in ('y', 'dx', 'dW', 'db'):
            if r64[q] is not None:
                worst[q, 'direct'] = max(worst.get((q, 'direct'), 0.0), R.rel_err(r32[q], r64[q]))
    for q in ('y', 'dx', 'dW', 'pool'):
        assert R.BARS[q, 'direct'] <= R.BARS[q, 'wino3x3'] and (q == 'pool' or R.BARS[q, 'wino3x3'] <= R.BARS[q, 'wino4x4'])
    for key, w in sorted(worst.items()):
        print('WORST %-20s %.3e -> bar %.0e' % (key, w, R.BARS[key]))
        assert math.isclose(R.BARS[key], _round_up_one_digit(8 * w), rel_tol=1e-9), (key, w)
    assert set(worst) == set(R.BARS) and max(R.BARS.values()) <= R.BAR_CAP == 5e-5


@pytest.mark.parametrize('row', ALL, ids=R.case_id)
def test_inputs_can_see_a_wrong_kernel(row):
    """Each mistake that applies to the row moves its quantity by more than 10 bars; operands of 11 mantissa bits by more than the bar."""
    fam, q, ref, _ = _measured(row)
    case = R.conv_case(row)
    assert 'g' in R.mistakes_of(row)
    for m in R.mistakes_of(row):
        wrong = R.case_ref(row, case, mistake=m)
        e = R.rel_err(wrong[0] if row.flags & R.F_POOL else wrong, ref)
        print('SENSITIVITY %-78s (%s) %-62s %.1f bars' % (R.case_id(row), m, R.MISTAKES[m], e / R.BARS[q, fam]))
        assert e > (1.0 if m == 'g' else 10.0) * R.BARS[q, fam], (m, R.MISTAKES[m], e)


def test_every_mistake_has_a_row():
    assert {m for row in ALL for m in R.mistakes_of(row)} == set(R.MISTAKES)
