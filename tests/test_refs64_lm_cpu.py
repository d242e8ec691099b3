"""Pins tests/refs64_lm.py (CPU only): the float64 window reference against a chain of ``nn.LSTMCell`` in double through autograd; for every
input of tests/test_lmseq_kernels_gpu.py, that torch's own fp32 run of the reference stays within a quarter of the bar the HIP kernels are
held to there, and that the input can see a wrong kernel; that ``LM_CASES`` covers what it says it covers and is closed under
re2e_lmseq_plan on a 256-CU chip (no device is touched)."""
import functools
import os

import pytest
import torch

import refs64_lm as R

IDS = [R.case_id(row) for row in R.LM_CASES]


@functools.lru_cache(maxsize=None)
def _refs(T, B, H, last):
    case = R.table_case((T, B, H))
    return case, R.case_ref(case, last), R.case_ref(case, last, torch.float32)


def test_reference_reproduces_a_chain_of_lstm_cells_in_double():
    """h, c of every step and, through autograd, the gradients of the input, of both biases, of W_ih, W_hh and of the initial state, with
    a gradient flowing in through the final state; then what lm_window_ref derives by itself (d(gates), dh0, dc0) against the same run."""
    T, B, I, H = 6, 5, 7, 9
    g = torch.Generator().manual_seed(5)
    cell = torch.nn.LSTMCell(I, H).double()
    for p in cell.parameters():
        p.data = R.rnd(g, *p.shape, scale=0.4).double()
    x = R.rnd(g, T, B, I).double().requires_grad_(True)
    h0, c0 = torch.tanh(R.rnd(g, B, H)).double().requires_grad_(True), R.rnd(g, B, H).double().requires_grad_(True)
    dy, dh_last, dc_last = (R.rnd(g, *s, scale=0.3).double() for s in ((T, B, H), (B, H), (B, H)))
    h, c, hs, cs = h0, c0, [], []
    for t in range(T):
        h, c = cell(x[t], (h, c))
        hs.append(h)
        cs.append(c)
    ((torch.stack(hs) * dy).sum() + (h * dh_last).sum() + (c * dc_last).sum()).backward()
    with torch.no_grad():
        xg = x @ cell.weight_ih.t() + cell.bias_ih + cell.bias_hh
    r = R.lm_window_ref(xg, cell.weight_hh, h0, c0, dy, dh_last, dc_last)
    assert R.rel_err(r['h'], torch.stack(hs)) <= 1e-12 and R.rel_err(r['c'], torch.stack(cs)) <= 1e-12
    assert R.rel_err(r['dh0'], h0.grad) <= 1e-12 and R.rel_err(r['dc0'], c0.grad) <= 1e-12
    dg = r['dgates'].reshape(T * B, 4 * H)
    assert R.rel_err((dg @ cell.weight_ih.detach()).view(T, B, I), x.grad) <= 1e-12
    assert R.rel_err(dg.sum(0), cell.bias_ih.grad) <= 1e-12 and R.rel_err(dg.sum(0), cell.bias_hh.grad) <= 1e-12
    assert R.rel_err(dg.t() @ x.detach().reshape(T * B, I), cell.weight_ih.grad) <= 1e-12
    hprev = torch.cat([h0.detach().unsqueeze(0), r['h'][:-1]]).reshape(T * B, H)          # hbuf[0:T]
    assert R.rel_err(dg.t() @ hprev, cell.weight_hh.grad) <= 1e-12
    # without the final-state gradient the answer differs: the optional inputs are live
    r0 = R.lm_window_ref(xg, cell.weight_hh, h0, c0, dy)
    assert R.rel_err(r0['dgates'], r['dgates']) > 1e-3


def test_case_table_covers_what_it_says():
    assert len(set(IDS)) == len(IDS)
    rows = R.LM_CASES
    assert {r[2] for r in rows} == {1, 9, 10, 33, 66, 650} and {r[1] for r in rows} == {1, 3, 33, 65} and {r[0] for r in rows} == {1, 2, 5}
    assert (2, 3, 650) in {r[:3] for r in rows}
    multi = [r for r in rows if r[0] >= 2]
    for H in R.LM_H:          # every width runs more than one step, with more than one row tile, and on an odd-aligned W_hh or an odd width
        assert any(r[2] == H for r in multi) and any(r[2] == H and r[1] == 65 for r in rows)
    for flag in (3, 4, 5):
        assert {r[flag] for r in multi} == {True, False}, flag
    assert {(r[3], r[4]) for r in multi} == {(True, True), (True, False), (False, True), (False, False)}
    assert any(r[5] for r in multi if r[2] == 650) and any(r[5] for r in multi if r[2] < 650)


@pytest.mark.parametrize('row', R.LM_CASES, ids=IDS)
def test_fp32_run_of_the_reference_stays_within_a_quarter_of_the_bar(row):
    T, B, H, last = row[:4]
    case, r64, r32 = _refs(T, B, H, last)
    for name, bar in R.QUANTITIES:
        assert torch.isfinite(r64[name]).all() and r64[name].abs().max() > 0, name
        e = R.margin_ok(name, r32[name], r64[name], bar)
        print('MARGIN %s %-7s fp32-cpu %.2e  bar %.0e' % (R.case_id(row), name, e, bar))


def test_inputs_can_see_a_wrong_kernel():
    """Mistakes a step kernel can make, made on the inputs of the reference: each moves a checked quantity by more than 100 bars."""
    for row in ((5, 33, 33), (2, 3, 650), (5, 3, 9)):
        T, B, H = row
        case, r64, _ = _refs(T, B, H, True)
        worst = {}
        w = case['whh'].clone()
        w[:, H - 1] = 0                                             # the K remainder of the forward product dropped
        worst['last k of h W_hh^T dropped'] = R.lm_window_ref(case['xg'], w, case['h0'], case['c0'], case['dy'], case['dh_last'], case['dc_last'])
        worst['zero initial state'] = R.lm_window_ref(case['xg'], case['whh'], torch.zeros(B, H), torch.zeros(B, H), case['dy'], case['dh_last'], case['dc_last'])
        worst['final-state gradient ignored'] = R.case_ref(case, False)
        perm = torch.cat([torch.arange(H, 2 * H), torch.arange(0, H), torch.arange(2 * H, 4 * H)])
        worst['input and forget gate swapped'] = R.lm_window_ref(case['xg'][:, :, perm], case['whh'][perm], case['h0'], case['c0'], case['dy'], case['dh_last'], case['dc_last'])
        for what, wrong in worst.items():
            names = [n for n, _ in R.QUANTITIES if not (what.startswith('input and forget') and n in ('gates', 'dgates'))]
            bars = max(R.rel_err(wrong[n], r64[n]) / dict(R.QUANTITIES)[n] for n in names)
            print('SENSITIVITY T%d-B%d-H%d %-34s %.1f bars' % (T, B, H, what, bars))
            assert bars > 100.0, (row, what, bars)


def test_cases_are_closed_under_the_plans():
    """No device is touched (cus = 256): every case's plans are the declared forms, every form a plan names over a sweep of shapes is
    declared and has a case, and the plan's grid covers the shape with the tile it names."""
    from robust_e2e_gan_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    declared = set()
    for T, B, H, _, _, _ in R.LM_CASES:
        for backward in (False, True):
            declared.add(R.plan_key(lib.lmseq_plan(T, B, H, backward=backward, cus=256)))
    assert declared == set(R.LM_PLANS)
    named = set()
    for B in (1, 3, 33, 64, 65, 256, 2048, 4096):
        for H in (1, 9, 10, 33, 66, 512, 650, 1024, 2048):
            for T in (1, 35):
                for backward in (False, True):
                    p = lib.lmseq_plan(T, B, H, backward=backward, cus=256)
                    named.add(R.plan_key(p))
                    gx, gy, gz = (int(v) for v in p['grid'].split('x'))
                    assert gz == 1 and gx * int(p['units']) >= H > (gx - 1) * int(p['units']) and gy * int(p['rows']) >= B > (gy - 1) * int(p['rows']), p
                    assert p['mfma'] == '16x16x4' and int(p['acc']) >= 2 and int(p['launches']) == T and 0 < int(p['lds']) <= 65536, p
    assert named == declared
    with pytest.raises(lib.Re2eError):
        lib.lmseq_plan(0, 3, 8, cus=256)
    with pytest.raises(lib.Re2eError):
        lib.lmseq_plan(35, 65536, 4096, cus=256)          # gates beyond 32-bit element offsets: an error code, not a plan
    so = lib.load()
    assert so.re2e_lmseq_workspace_bytes(3, 650) >= 3 * 650 * 4


def test_model_reference_reproduces_the_fixture_window(golden_dir):
    """lm_model_ref in double against what the reference itself computed in fp32 (tests/golden/lm_train_tiny.npz): per-step losses, final
    state and the gradients of all 11 parameters -- the yardstick of the dropout test is the model the fixture was written by."""
    import numpy as np
    fx = dict(np.load(os.path.join(golden_dir, 'lm_train_tiny.npz')))
    params = {k: torch.from_numpy(fx['lm.predictor.' + k]) for k in R.PARAM_NAMES}
    r = R.lm_model_ref(params, fx['win.xs'], fx['win.ts'])
    assert R.rel_err(r['losses'], torch.from_numpy(fx['win.losses'])) <= 1e-5
    for k in R.STATE_KEYS:
        assert R.rel_err(r[k], torch.from_numpy(fx['win.state.' + k])) <= 1e-5, k
    for k in R.PARAM_NAMES:
        assert R.rel_err(r['grad.' + k], torch.from_numpy(fx['win.grad.predictor.' + k])) <= 1e-5, k
