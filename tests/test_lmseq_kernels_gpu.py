"""The step kernels of csrc/lmseq.hip against the float64 reference of tests/refs64_lm.py, through the C ABI (re2e_lmseq_fwd / _bwd), at the
smallest shapes where they can go wrong (refs64_lm.LM_CASES: K and unit-tile remainders, odd widths, the recipe's H = 650, partial row
tiles on both sides of the 64-row tile, 1 / 2 / 5 steps, a non-zero initial state, with and without the gradient through the final state,
with and without the gradient of the initial state asked for, W_hh 4 bytes off a 16-byte boundary); every row first asserts that the
library's plans for its shape are the forms the table declares.  re2e_sgd_step against float64.

Every call: h / c blocks 1 .. T, dh0, dc0 and the workspace are NaN before it (a kernel must write all of what it owns and read nothing it
has not written), forward and backward run twice on fresh copies of the gates, block 0 of hbuf / cbuf must come back bit-identical.  The
bars are the project's own (test_recurrence_kernels_gpu.py): 1e-4 of the tensor's max for h, c and the activated gates, 2e-4 for the
gradients; each quantity first asserts that torch's fp32 CPU run of the reference stays within a quarter of its bar, then prints both
distances.  GPU only.

Measured on an MI355X when the module was written, worst case over the table, HIP / fp32 on the CPU (of the tensor's max):
    h 8.7e-7 / 3.6e-7, c 5.0e-7 / 1.9e-7, gates 1.3e-6 / 5.2e-7                                   (bar 1e-4)
    d(gates) 1.5e-6 / 3.4e-7, dh0 1.8e-6 / 1.6e-6, dc0 3.0e-6 / 4.9e-7                             (bar 2e-4)
every worst case at H = 650 (the longest chains); the small widths sit at 1e-7 .. 5e-7.  re2e_sgd_step: 4.6e-8 / 4.6e-8 (bar 1e-6).
Two orders inside the bars: where fp32 arithmetic puts a k-ordered chain of 650 / 2600 terms."""
import functools

import pytest
import torch

import refs64_lm as R
from test_loss_kernels_gpu import DEV, _held, _ops

pytestmark = pytest.mark.gpu

NAN = float('nan')


@functools.lru_cache(maxsize=None)
def _refs(T, B, H, last):
    case = R.table_case((T, B, H))
    return case, R.case_ref(case, last), R.case_ref(case, last, torch.float32)


def _run_hip(lib, case, last, out, misalign):
    """re2e_lmseq_fwd twice, then re2e_lmseq_bwd twice from the second forward's state -> dict of CPU tensors (the names of lm_window_ref,
    plus block 0 of hbuf / cbuf)."""
    T, B, H = case['T'], case['B'], case['H']
    if misalign:                                                              # 4 bytes off a 16-byte boundary
        store = torch.empty(4 * H * H + 4, device=DEV)
        whh = store[1:1 + 4 * H * H].view(4 * H, H)
        whh.copy_(case['whh'])
        assert whh.data_ptr() % 16 == 4
    else:
        whh = case['whh'].to(DEV)
        assert whh.data_ptr() % 16 == 0
    xg0 = case['xg'].to(DEV)
    dy = case['dy'].to(DEV)
    dh_last, dc_last = (case[k].to(DEV) if last else None for k in ('dh_last', 'dc_last'))
    wsb = lib.query('re2e_lmseq_workspace_bytes', B, H)
    assert wsb >= B * H * 4
    hbuf, cbuf = torch.empty(T + 1, B, H, device=DEV), torch.empty(T + 1, B, H, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    for _ in range(2):
        gates = xg0.clone()
        ws = torch.full((wsb // 4 + 16,), NAN, device=DEV)                    # poisoned: nothing may be read before it is written
        hbuf.fill_(NAN)
        cbuf.fill_(NAN)
        hbuf[0].copy_(case['h0'])
        cbuf[0].copy_(case['c0'])
        lib.call('re2e_lmseq_fwd', gates.data_ptr(), whh.data_ptr(), hbuf.data_ptr(), cbuf.data_ptr(), T, B, H, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    for _ in range(2):
        G = gates.clone()
        ws = torch.full((wsb // 4 + 16,), NAN, device=DEV)
        dh0, dc0 = (torch.full((B, H), NAN, device=DEV) if out else None for _ in range(2))
        lib.call('re2e_lmseq_bwd', G.data_ptr(), whh.data_ptr(), dy.data_ptr(), p(dh_last), p(dc_last), cbuf.data_ptr(), p(dh0), p(dc0), T, B, H,
                 ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    assert torch.isnan(ws[wsb // 4:]).all(), 'written beyond re2e_lmseq_workspace_bytes'
    return dict(h=hbuf[1:].cpu(), c=cbuf[1:].cpu(), gates=gates.cpu(), dgates=G.cpu(), dh0=dh0.cpu() if out else None, dc0=dc0.cpu() if out else None,
                block0=torch.stack([hbuf[0], cbuf[0]]).cpu())


@pytest.mark.parametrize('row', R.LM_CASES, ids=R.case_id)
def test_lmseq_against_float64(row):
    ops, lib = _ops()
    T, B, H, last, out, misalign = row
    assert R.plan_key(lib.lmseq_plan(T, B, H)) == R.LM_PLANS[0] and R.plan_key(lib.lmseq_plan(T, B, H, backward=True)) == R.LM_PLANS[1]
    case, r64, r32 = _refs(T, B, H, last)
    got = _run_hip(lib, case, last, out, misalign)
    assert torch.equal(got['block0'], torch.stack([case['h0'], case['c0']])), 'block 0 of hbuf / cbuf is the caller\'s: it must stay untouched'
    for name, bar in R.QUANTITIES:
        if got[name] is None:
            continue
        assert torch.isfinite(got[name]).all(), '%s %s: not finite where the reference is' % (R.case_id(row), name)
        _held(R.case_id(row), name, got[name], r64[name], r32[name], bar)


def test_sgd_step_against_float64():
    """p -= lr * stats[1] * g over a length that is no multiple of the block, with a clip coefficient below 1, without stats (coefficient
    1), and skipped bit-identically when stats[2] == 0.  Bar 1e-6 of max |p|: three fp32 roundings (lr * coefficient, the product, the
    difference) of 6e-8 each, times four for the quarter the fp32 CPU run has to stay within."""
    ops, lib = _ops()
    g = torch.Generator().manual_seed(11)
    n = 2 * 4096 * 256 + 13                                                  # more than one sweep of the grid, odd tail
    p0, gr = R.rnd(g, n), R.rnd(g, n, scale=0.3)
    for stats, lr in (([7.0, 0.37, 1.0, 7.0, 1.0, 1.0], 1.0), ([1.0, 1.0, 1.0, 1.0, 1.0, 1.0], 0.25), (None, 0.5)):
        st = torch.tensor(stats) if stats is not None else torch.tensor([0.0, 1.0, 1.0])
        p = p0.to(DEV)
        lib.call('re2e_sgd_step', p.data_ptr(), gr.to(DEV).data_ptr(), n, lr, st.to(DEV).data_ptr() if stats is not None else None)
        r64, r32 = R.sgd_ref(p0, gr, lr, st), R.sgd_ref(p0, gr, lr, st, torch.float32)
        _held('sgd lr=%g coef=%g' % (lr, float(st[1])), 'p', p.cpu(), r64, r32, 1e-6)
    for bad in (0.0,):
        st = torch.tensor([float('inf'), 0.5, bad, float('inf'), 1.0, bad])
        p = p0.to(DEV)
        lib.call('re2e_sgd_step', p.data_ptr(), gr.to(DEV).data_ptr(), n, 1.0, st.to(DEV).data_ptr())
        assert torch.equal(p.cpu(), p0), 'stats[2] == 0: the update must be skipped, p bit-identical'
