"""The cell-step kernels of csrc/fsrnn.hip against the float64 reference of tests/refs64_fsrnn.py, through the C ABI (re2e_fsrnn_fwd / _bwd),
at the smallest shapes where they can go wrong (refs64_fsrnn.FS_CASES); every row first asserts that the library's plans for its shape are
the forms the table declares.  re2e_lm_lstm_cell_zo against float64.

Every call: the states' blocks 1 .. T, hd, the gradients of the initial state and the workspace are NaN before it (a kernel must write all
of what it owns and read nothing it has not written), block 0 of the last fast cell and of the slow cell must come back bit-identical.  The
bars are the project's own: 1e-4 of the tensor's max for states and activated gates, 2e-4 for the gradients; each quantity first asserts
that torch's fp32 CPU run of the reference stays within a quarter of its bar, then prints both distances.  GPU only."""
import functools

import pytest
import torch

import refs64_fsrnn as R
from test_loss_kernels_gpu import DEV, _held, _ops

pytestmark = pytest.mark.gpu

NAN = float('nan')


@functools.lru_cache(maxsize=None)
def _refs(row):
    masks, drop, last = row[4:7]
    case = R.table_case(row)
    return case, R.case_ref(case, masks, drop, last), R.case_ref(case, masks, drop, last, torch.float32)


def _run_hip(lib, case, masks, drop, last, misalign):
    T, B, H, L = case['T'], case['B'], case['H'], case['L']
    keep = []

    def dev(t):
        if misalign and t.dim() == 2:                                        # 4 bytes off a 16-byte boundary
            store = torch.empty(t.numel() + 4, device=DEV)
            v = store[1:1 + t.numel()].view(t.shape)
            v.copy_(t)
            assert v.data_ptr() % 16 == 4
        else:
            v = t.to(DEV)
        keep.append(v)
        return v

    W = [tuple(dev(w) for w in cell) for cell in case['W']]
    arrays = [lib.pointer_array([cell[i] for cell in W]) for i in range(4)]
    mh, mc = (case[k].to(DEV) if masks else None for k in ('mh', 'mc'))
    dm = case['dm'].to(DEV) if drop else None
    p = lambda t: None if t is None else t.data_ptr()
    gates = torch.full((L + 1, T, B, 4 * H), NAN, device=DEV)
    gates[0].copy_(case['xg'])
    hbuf, cbuf = torch.full((L + 1, T + 1, B, H), NAN, device=DEV), torch.full((L + 1, T + 1, B, H), NAN, device=DEV)
    for c, (h0, c0) in ((L - 1, case['state'][:2]), (L, case['state'][2:])):
        hbuf[c, 0].copy_(h0)
        cbuf[c, 0].copy_(c0)
    hd = torch.full((2, T, B, H), NAN, device=DEV) if drop else None
    wsb = lib.query('re2e_fsrnn_workspace_bytes', B, H)
    assert wsb >= 4 * B * H * 4
    ws = torch.full((wsb // 4 + 16,), NAN, device=DEV)
    lib.call('re2e_fsrnn_fwd', gates.data_ptr(), hbuf.data_ptr(), cbuf.data_ptr(), p(hd), arrays[0], arrays[1], arrays[2], arrays[3], p(mh), p(mc), p(dm),
             R.KEEP_H, R.KEEP_C, T, B, H, L, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    G = gates.clone()
    dy = case['dy'].to(DEV)
    d_last = [d.to(DEV) if last else None for d in case['d_last']]
    d0 = [torch.full((B, H), NAN, device=DEV) if last else None for _ in range(4)]
    lib.call('re2e_fsrnn_bwd', G.data_ptr(), cbuf.data_ptr(), arrays[0], arrays[1], p(mh), p(mc), p(dm), R.KEEP_H, R.KEEP_C, dy.data_ptr(),
             p(d_last[0]), p(d_last[1]), p(d_last[2]), p(d_last[3]), p(d0[0]), p(d0[1]), p(d0[2]), p(d0[3]), T, B, H, L, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    assert torch.isnan(ws[wsb // 4:]).all(), 'written beyond re2e_fsrnn_workspace_bytes'
    out = dict(h=hbuf[:, 1:].cpu(), c=cbuf[:, 1:].cpu(), gates=gates.cpu(), hd=hd.cpu() if drop else None, dgates=G.cpu(),
               block0=torch.stack([hbuf[L - 1, 0], cbuf[L - 1, 0], hbuf[L, 0], cbuf[L, 0]]).cpu(),
               unused0=torch.stack([hbuf[:L - 1, 0], cbuf[:L - 1, 0]]).cpu())
    out.update({k: (d.cpu() if d is not None else None) for k, d in zip(('d_fh0', 'd_fc0', 'd_sh0', 'd_sc0'), d0)})
    return out


@pytest.mark.parametrize('row', R.FS_CASES, ids=R.case_id)
def test_fsrnn_against_float64(row):
    ops, lib = _ops()
    T, B, H, L, masks, drop, last, misalign = row
    assert R.plan_key(lib.fsrnn_plan(T, B, H, L)) == R.FS_PLANS[0] and R.plan_key(lib.fsrnn_plan(T, B, H, L, backward=True)) == R.FS_PLANS[1]
    case, r64, r32 = _refs(row)
    got = _run_hip(lib, case, masks, drop, last, misalign)
    assert torch.equal(got['block0'], torch.stack(case['state'])), 'block 0 of the last fast cell and of the slow cell is the caller\'s'
    assert torch.isnan(got['unused0']).all(), 'block 0 of the other cells is not the kernels\' to write'
    for name, bar in R.QUANTITIES:
        if got[name] is None:
            continue
        assert torch.isfinite(got[name]).all(), '%s %s: not finite where the reference is' % (R.case_id(row), name)
        _held(R.case_id(row), name, got[name], r64[name], r32[name], bar)


@functools.lru_cache(maxsize=None)
def _cell_case(H):
    g = torch.Generator().manual_seed(300 + H)
    I = H + 3
    return dict(I=I, x=R.rnd(g, 64, I), w_ih=R.rnd(g, 4 * H, I, scale=I ** -0.5), w_hh=R.rnd(g, 4 * H, H, scale=H ** -0.5), b_ih=R.rnd(g, 4 * H, scale=0.3),
                b_hh=R.rnd(g, 4 * H, scale=0.3), h=torch.tanh(R.rnd(g, 64, H)), c=R.rnd(g, 64, H, scale=0.7))


@pytest.mark.parametrize('H', (10, 33, 650))
@pytest.mark.parametrize('n', (1, 5, 13, 33, 64))
def test_lm_lstm_cell_zo_against_float64(n, H):
    """With and without an input, with and without a previous state; the outputs are NaN beforehand (every element is written)."""
    ops, lib = _ops()
    cs = _cell_case(H)
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in cs.items()}
    for with_x in (True, False):
        for with_state in (True, False):
            if not with_x and not with_state and n > 5:
                continue          # (bias alone: every row the same; two sizes are enough)
            x, h, c = (cs['x'][:n] if with_x else None), (cs['h'][:n] if with_state else None), (cs['c'][:n] if with_state else None)
            xd, hd_, cd = (d['x'][:n].contiguous() if with_x else None), (d['h'][:n].contiguous() if with_state else None), (d['c'][:n].contiguous() if with_state else None)
            ho, co = torch.full((n, H), NAN, device=DEV), torch.full((n, H), NAN, device=DEV)
            p = lambda t: None if t is None else t.data_ptr()
            lib.call('re2e_lm_lstm_cell_zo', p(xd), cs['I'], None, 0, cs['I'], d['w_ih'].data_ptr(), d['w_hh'].data_ptr(), d['b_ih'].data_ptr(),
                     d['b_hh'].data_ptr(), p(hd_), p(cd), n, H, R.KEEP_H, R.KEEP_C, ho.data_ptr(), co.data_ptr())
            args = (x, cs['w_ih'], cs['w_hh'], cs['b_ih'], cs['b_hh'], h, c, R.KEEP_H, R.KEEP_C)
            if x is None and h is None:
                h64, c64 = (t[:1].expand(n, H) for t in R.cell_zo_ref(*args))
                h32, c32 = (t[:1].expand(n, H) for t in R.cell_zo_ref(*args, dtype=torch.float32))
            else:
                (h64, c64), (h32, c32) = R.cell_zo_ref(*args), R.cell_zo_ref(*args, dtype=torch.float32)
            what = 'n%d-H%d%s%s' % (n, H, '-x' if with_x else '', '-state' if with_state else '')
            _held(what, 'h', ho.cpu(), h64, h32, R.BAR_OUT)
            _held(what, 'c', co.cpu(), c64, c32, R.BAR_OUT)


def test_lm_lstm_cell_zo_gathers_and_poisons_bad_ids():
    """x as an embedding table gathered by ids: rows equal the dense call on the gathered rows, and an id outside the table gives a NaN row."""
    ops, lib = _ops()
    H, n = 33, 5
    cs = _cell_case(H)
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in cs.items()}
    ids = torch.tensor([3, 63, 0, 64, -1], dtype=torch.int32)
    ho, co = torch.full((n, H), NAN, device=DEV), torch.full((n, H), NAN, device=DEV)
    hp, cp = d['h'][:n].contiguous(), d['c'][:n].contiguous()
    lib.call('re2e_lm_lstm_cell_zo', d['x'].data_ptr(), cs['I'], ids.to(DEV).data_ptr(), 64, cs['I'], d['w_ih'].data_ptr(), d['w_hh'].data_ptr(),
             d['b_ih'].data_ptr(), d['b_hh'].data_ptr(), hp.data_ptr(), cp.data_ptr(), n, H, R.KEEP_H, R.KEEP_C, ho.data_ptr(), co.data_ptr())
    ho, co = ho.cpu(), co.cpu()
    assert torch.isnan(ho[3:]).all() and torch.isnan(co[3:]).all() and torch.isfinite(ho[:3]).all() and torch.isfinite(co[:3]).all()
    args = (cs['x'][[3, 63, 0]], cs['w_ih'], cs['w_hh'], cs['b_ih'], cs['b_hh'], cs['h'][:3], cs['c'][:3], R.KEEP_H, R.KEEP_C)
    (h64, c64), (h32, c32) = R.cell_zo_ref(*args), R.cell_zo_ref(*args, dtype=torch.float32)
    _held('gather', 'h', ho[:3], h64, h32, R.BAR_OUT)
    _held('gather', 'c', co[:3], c64, c32, R.BAR_OUT)
