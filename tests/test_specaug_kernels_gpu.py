"""csrc/specaug.hip (re2e_spec_augment_fwd / _bwd) through the C ABI (lib.call) against the float64 reference of tests/refs64_specaug.py, which
resizes every segment with ``F.interpolate`` itself and takes dx from autograd.  The forward is held to refs64_feat.BAR_FBANK_OUT (1e-5 of the
tensor's max), the backward to BAR_FBANK_GRAD (1e-4), each behind ``margin_ok``: the fp32 CPU run of the reference stays within a quarter of the
bar on the same input.  The cases (refs64_specaug.cases) are the smallest at which each branch of the kernels can go wrong."""
import numpy as np
import pytest
import torch

import refs64_specaug as RS
from test_refs64_specaug_cpu import CASES, ref_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _run(lib, x, dy, plan, nF, nT, y=None, dx=None):
    """x, dy on the device (either may be None); plan: host int array.  Returns (y, dx)."""
    pd = torch.from_numpy(np.ascontiguousarray(plan, dtype=np.int32)).to(DEV)
    R, Tp, F = (x if x is not None else dy).shape
    if x is not None:
        y = torch.full_like(x, float('nan')) if y is None else y
        lib.call('re2e_spec_augment_fwd', x.data_ptr(), pd.data_ptr(), R, Tp, F, nF, nT, y.data_ptr())
    if dy is not None:
        dx = torch.full_like(dy, float('nan')) if dx is None else dx
        lib.call('re2e_spec_augment_bwd', dy.data_ptr(), pd.data_ptr(), R, Tp, F, nF, nT, dx.data_ptr())
    torch.cuda.synchronize()
    return y, dx


def _check(name, y, dx, x, dy, plan, y64, dx64, f32=None):
    ey, ed = RS.rel_err(y, y64), RS.rel_err(dx, dx64)
    print('ERR %-18s y %.2e (bar %.0e)  dx %.2e (bar %.0e)' % (name, ey, RS.BAR_FBANK_OUT, ed, RS.BAR_FBANK_GRAD))
    assert ey <= RS.BAR_FBANK_OUT and ed <= RS.BAR_FBANK_GRAD, (name, ey, ed)
    for r in range(x.shape[0]):                            # the padding comes through unchanged, bit for bit, forward and backward
        T = int(plan[r, 0])
        assert torch.equal(y[r, T:].cpu(), x[r, T:]) and torch.equal(dx[r, T:].cpu(), dy[r, T:]), (name, r)


def test_geometry_is_what_the_cases_were_built_for():
    from robust_e2e_gan_amd import lib
    ft, bt, mm, ch = (lib.query('re2e_spec_augment_geometry', k) for k in range(4))
    assert (ft, bt) == (32, 32) and set(RS.cases(ft, bt)) == set(CASES)      # 'tile32_plus1' / 'tile32_x2' sit on both kernels' tiling
    assert mm == 8 and ch < 199                            # 'clamped' row 3 sums more output frames into one source frame than are staged
    assert lib.query('re2e_spec_augment_geometry', 4) == -1


@pytest.mark.parametrize('name', sorted(CASES))
def test_case(name):
    from robust_e2e_gan_amd import lib
    c = CASES[name]
    x, dy, plan, y64, dx64 = ref_of(name)
    y32, dx32 = RS.specaug_ref(x, plan, c['nF'], c['nT'], dy, dtype=torch.float32)
    RS.margin_ok(name + ' y', y32, y64, RS.BAR_FBANK_OUT)
    RS.margin_ok(name + ' dx', dx32, dx64, RS.BAR_FBANK_GRAD)
    # the kernels get the plan AS IT IS (outside its ranges for 'clamped'); the reference ran on the clamped one
    y, dx = _run(lib, x.to(DEV), dy.to(DEV), c['plan'], c['nF'], c['nT'])
    _check(name, y, dx, x, dy, plan, y64, dx64)
    if c['exact']:
        assert torch.equal(y.cpu(), x) and torch.equal(dx.cpu(), dy), name
    if name == 'full_F':
        for r in range(x.shape[0]):
            T = int(plan[r, 0])
            assert not y[r, :T].any() and not dx[r, :T].any()
    if name == 'clamped':                                  # the same bits as the call given the clamped plan
        y2, dx2 = _run(lib, x.to(DEV), dy.to(DEV), plan, c['nF'], c['nT'])
        assert torch.equal(y, y2) and torch.equal(dx, dx2)


def test_scalar_form_on_unaligned_pointers_equals_the_vector_form():
    """F % 4 == 0 on pointers that are not 16-byte aligned takes the scalar kernels: the same values, bit for bit."""
    from robust_e2e_gan_amd import lib
    c = CASES['width_F80']
    x, dy, plan, y64, dx64 = ref_of('width_F80')
    y, dx = _run(lib, x.to(DEV), dy.to(DEV), c['plan'], c['nF'], c['nT'])
    n = x.numel()
    bufs = [torch.full((n + 1,), float('nan'), device=DEV) for _ in range(4)]
    xs, ds, ys, dxs = (b[1:].view(x.shape) for b in bufs)
    assert xs.data_ptr() % 16 == 4
    xs.copy_(x)
    ds.copy_(dy)
    _run(lib, xs, ds, c['plan'], c['nF'], c['nT'], y=ys, dx=dxs)
    assert torch.equal(ys, y), 'forward'
    assert torch.equal(dxs, dx), 'backward'
    assert all(torch.isnan(b[0]).item() for b in bufs[2:])


def test_production_shape():
    """(32, 800, 80) with plans drawn for ESPnet's defaults, ragged lengths.  Its data vary slowly along time: on white noise the fp32 CPU run
    of the reference is 4.1e-5 (y) and 2.9e-5 (dx) of the max from float64 at this length and fails both preconditions."""
    from robust_e2e_gan_amd import lib
    from robust_e2e_gan_amd.data import spec_augment as sa
    lens = [800 - 23 * (b % 9) - b for b in range(32)]
    plan = sa.draw_plan(4, 17, 0, lens, 80, '5,30,2,40,2')
    assert np.array_equal(RS.clamp_plan(plan, 800, 80, 2, 2), plan) and all(int(c) > 0 for c in plan[:, 1])
    case = dict(shape=(32, 800, 80), nF=2, nT=2, plan=plan)
    x, dy, _ = RS.case_tensors(case, seed=5, smooth=True)      # (why smooth: refs64_specaug.case_tensors)
    y64, dx64 = RS.specaug_ref(x, plan, 2, 2, dy)
    y32, dx32 = RS.specaug_ref(x, plan, 2, 2, dy, dtype=torch.float32)
    RS.margin_ok('production y', y32, y64, RS.BAR_FBANK_OUT)
    RS.margin_ok('production dx', dx32, dx64, RS.BAR_FBANK_GRAD)
    y, dx = _run(lib, x.to(DEV), dy.to(DEV), plan, 2, 2)
    _check('production', y, dx, x, dy, plan, y64, dx64)


def test_backward_is_deterministic():
    from robust_e2e_gan_amd import lib
    for name in ('ragged', 'clamped', 'width_F83'):
        c = CASES[name]
        x, dy, plan, _, _ = ref_of(name)
        g = dy.to(DEV)
        a = _run(lib, None, g, c['plan'], c['nF'], c['nT'])[1]
        b = _run(lib, None, g, c['plan'], c['nF'], c['nT'])[1]
        assert torch.equal(a, b), name


def test_refusals_write_nothing():
    """Every refusal of the header comment carries a word of its message and leaves the output at its sentinel."""
    from robust_e2e_gan_amd import lib
    x = torch.randn(2, 9, 4, device=DEV)
    out = torch.full_like(x, 3.5)
    pd = torch.tensor([[9, 0, 0, 0, 0, 0, 0]] * 2, dtype=torch.int32, device=DEV)
    good = dict(a=x.data_ptr(), p=pd.data_ptr(), R=2, Tp=9, F=4, nF=1, nT=1, b=out.data_ptr())
    bad = [(dict(b=x.data_ptr()), 'in place'), (dict(R=0), 'non-positive'), (dict(Tp=0), 'non-positive'), (dict(F=-1), 'non-positive'),
           (dict(nF=9), 'RE2E_SPECAUG_MAX_MASKS'), (dict(nT=9), 'RE2E_SPECAUG_MAX_MASKS'), (dict(nF=-1), 'RE2E_SPECAUG_MAX_MASKS'),
           (dict(a=None), 'null'), (dict(p=None), 'null'), (dict(b=None), 'null')]
    for entry in ('re2e_spec_augment_fwd', 're2e_spec_augment_bwd'):
        for change, word in bad:
            a = dict(good, **change)
            with pytest.raises(lib.Re2eError) as e:
                lib.call(entry, a['a'], a['p'], a['R'], a['Tp'], a['F'], a['nF'], a['nT'], a['b'])
            assert word in str(e.value) and entry in str(e.value), (entry, change, str(e.value))
    torch.cuda.synchronize()
    assert (out == 3.5).all(), 'a refused call wrote an output'
    lib.call('re2e_spec_augment_fwd', *[good[k] for k in ('a', 'p', 'R', 'Tp', 'F', 'nF', 'nT', 'b')])      # and the good call runs
    torch.cuda.synchronize()
    assert torch.equal(out, x)


def test_op_validates_on_the_host_and_differentiates():
    """ops.spec_augment: a plan outside its ranges is refused on the host by name; autograd reaches the backward kernel."""
    from robust_e2e_gan_amd import lib, ops
    from robust_e2e_gan_amd.data import spec_augment as sa
    c = CASES['ragged']
    x, dy, plan, y64, dx64 = ref_of('ragged')
    xd = x.to(DEV).requires_grad_(True)
    y = ops.spec_augment(xd, sa.Plan(c['plan'], c['nF']))
    y.backward(dy.to(DEV))
    y2 = ops.spec_augment(xd.detach(), c['plan'], nF=c['nF'])
    torch.cuda.synchronize()
    _check('op', y.detach(), xd.grad, x, dy, plan, y64, dx64)
    assert torch.equal(y2, y.detach())
    for args, word in (((xd, CASES['clamped']['plan'][:3, :], 1), 'T_r'), ((xd, c['plan'][:2], 1), 'plan rows'), ((xd, c['plan']), 'nF'),
                       ((x, c['plan'], 1), 'GPU only')):
        with pytest.raises(lib.Re2eError) as e:
            ops.spec_augment(*args)
        assert word in str(e.value), str(e.value)
