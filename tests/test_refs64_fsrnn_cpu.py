"""Pins tests/refs64_fsrnn.py (CPU only): the float64 window reference against a chain of ``nn.LSTMCell`` in double with explicit zoneout
and dropout masks through autograd, and against what the reference model itself computed (tests/golden/fsrnn_tiny.npz, ``win.*``); for
every input of tests/test_fsrnn_kernels_gpu.py, that torch's own fp32 run of the reference stays within a quarter of the bar the HIP kernels
are held to there; that ``FS_CASES`` covers what it says it covers and is closed under re2e_fsrnn_plan on a 256-CU chip (no device is
touched); and the host side of the feature: what the model refuses, its state_dict names and the trainer's dispatch."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch

import refs64_fsrnn as R

IDS = [R.case_id(row) for row in R.FS_CASES]


@functools.lru_cache(maxsize=None)
def _refs(row):
    masks, drop, last = row[4:7]
    case = R.table_case(row)
    return case, R.case_ref(case, masks, drop, last), R.case_ref(case, masks, drop, last, torch.float32)


@pytest.mark.parametrize('L,masks', [(2, True), (3, False), (4, True)])
def test_reference_reproduces_a_chain_of_lstm_cells_in_double(L, masks):
    """States of every cell and step and, through autograd, the gradients of the pre-activations' input, of the initial state and of every
    cell's parameters, with a gradient flowing in through the final state -- against nn.LSTMCell modules wired as fsrnn.py:96-127 wires them."""
    T, B, H = 4, 3, 5
    case = R.fs_case(T, B, H, L, seed=77 + L)
    dbl = lambda t: t.double()
    cells = [torch.nn.LSTMCell(H, H).double() for _ in range(L + 1)]
    for cell, w in zip(cells, case['W']):
        for p, v in zip((cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh), w):
            p.data = dbl(v).clone()
    xg = dbl(case['xg']).requires_grad_(True)
    st0 = [dbl(s).clone().requires_grad_(True) for s in case['state']]
    mh = dbl(case['mh']) if masks else torch.full((L + 1, T, B, H), R.KEEP_H, dtype=torch.float64)
    mc = dbl(case['mc']) if masks else torch.full((L + 1, T, B, H), R.KEEP_C, dtype=torch.float64)
    dm = dbl(case['dm']) if masks else None
    zo = lambda new, old, m: new * m + (-m + 1.) * old
    Fh, Fc, Sh, Sc = st0
    ys, hs = [], {}
    zero_in = torch.zeros(B, H, dtype=torch.float64)
    for t in range(T):
        # fast cell 0 with its input product hoisted: nn.LSTMCell(x) == cell on pre-activations xg + h W_hh^T with a zero input and zero biases
        pre = xg[t] + Fh @ cells[0].weight_hh.t()
        hn, cn, _ = R._cell(pre, Fc)
        Fh, Fc = zo(hn, Fh, mh[0, t]), zo(cn, Fc, mc[0, t])
        hs[0, t] = Fh
        hn, cn = cells[L](Fh * dm[0, t] if dm is not None else Fh, (Sh, Sc))
        Sh, Sc = zo(hn, Sh, mh[L, t]), zo(cn, Sc, mc[L, t])
        hs[L, t] = Sh
        hn, cn = cells[1](Sh * dm[1, t] if dm is not None else Sh, (Fh, Fc))
        Fh, Fc = zo(hn, Fh, mh[1, t]), zo(cn, Fc, mc[1, t])
        hs[1, t] = Fh
        for k in range(2, L):
            hn, cn = cells[k](Fh * 0.0, (Fh, Fc))
            Fh, Fc = zo(hn, Fh, mh[k, t]), zo(cn, Fc, mc[k, t])
            hs[k, t] = Fh
        ys.append(Fh)
    loss = (torch.stack(ys) * dbl(case['dy'])).sum() + sum((s * dbl(d)).sum() for s, d in zip((Fh, Fc, Sh, Sc), case['d_last']))
    loss.backward()
    r = R.fs_window_ref(case['xg'], case['W'], case['state'], case['mh'] if masks else R.KEEP_H, case['mc'] if masks else R.KEEP_C, case['dm'] if masks else None,
                        L, case['dy'], case['d_last'])
    assert R.rel_err(r['y'], torch.stack(ys)) <= 1e-12
    for (c, t), h in hs.items():
        assert R.rel_err(r['h'][c, t], h) <= 1e-12, (c, t)
    assert R.rel_err(r['dgates'][0], xg.grad) <= 1e-12
    for k, s in zip(('d_fh0', 'd_fc0', 'd_sh0', 'd_sc0'), st0):
        assert R.rel_err(r[k], s.grad) <= 1e-12, k
    M = T * B
    for c, cell in enumerate(cells):
        dg = r['dgates'][c].reshape(M, 4 * H)
        assert R.rel_err(r['dW'][c][1], cell.weight_hh.grad) <= 1e-12, c
        # the products the autograd function accumulates after the loop (ops.FsrnnSeqFn), from the buffers of the contract
        h_prev = torch.cat([dbl(case['state'][0 if c == 0 else 2]).unsqueeze(0), r['h'][L - 1 if c == 0 else L][:-1]]) if c in (0, L) else r['h'][c - 1]
        assert R.rel_err(dg.t() @ h_prev.reshape(M, H), cell.weight_hh.grad) <= 1e-12, c
        if c in (1, L):
            x_in = r['hd'][0 if c == L else 1] if masks else r['h'][0 if c == L else L]
            assert R.rel_err(dg.t() @ x_in.reshape(M, H), cell.weight_ih.grad) <= 1e-12, c
        if c >= 1:
            assert R.rel_err(dg.sum(0), cell.bias_ih.grad) <= 1e-12 and R.rel_err(dg.sum(0), cell.bias_hh.grad) <= 1e-12, c
        if 2 <= c < L:
            assert float(cell.weight_ih.grad.abs().max()) == 0.0          # a zero tensor, not None
    # without the final-state gradient the answer differs: the optional inputs are live
    r0 = R.fs_window_ref(case['xg'], case['W'], case['state'], R.KEEP_H, R.KEEP_C, None, L, case['dy'])
    assert R.rel_err(r0['dgates'], r['dgates']) > 1e-3


@pytest.mark.parametrize('L', (2, 3))
def test_model_reference_reproduces_the_fixture_window(golden_dir, L):
    """fs_model_ref in double against what the reference itself computed in fp32 (evaluation mode, gradients enabled): per-step losses, the
    final state and the gradients of every parameter."""
    fx = dict(np.load(os.path.join(golden_dir, 'fsrnn_tiny.npz')))
    pre = 'L%d.' % L
    params = {k: torch.from_numpy(fx[pre + 'lm.predictor.' + k]) for k in R.param_names(L)}
    r = R.fs_model_ref(params, fx[pre + 'win.xs'], fx[pre + 'win.ts'], L, 0.9, 0.5)
    assert R.rel_err(r['losses'], torch.from_numpy(fx[pre + 'win.losses'])) <= 1e-5
    for k in R.STATE_KEYS:
        assert R.rel_err(r[k], torch.from_numpy(fx[pre + 'win.state.' + k])) <= 1e-5, k
    for k in R.param_names(L):
        want = torch.from_numpy(fx[pre + 'win.grad.predictor.' + k])
        if float(want.abs().max()) == 0.0:
            assert k.endswith('weight_ih') and float(r['grad.' + k].abs().max()) == 0.0, k
        else:
            assert R.rel_err(r['grad.' + k], want) <= 2e-5, k


def test_case_table_covers_what_it_says():
    assert len(set(IDS)) == len(IDS)
    rows = R.FS_CASES
    assert {r[2] for r in rows} == {1, 9, 33, 66, 650} and {r[1] for r in rows} == {1, 3, 65} and {r[0] for r in rows} == {1, 2, 5}
    assert {r[3] for r in rows} == {2, 3, 4} and (2, 3, 650) in {r[:3] for r in rows}
    multi = [r for r in rows if r[0] >= 2]
    for H in R.FS_H:          # every width runs more than one step and more than one row tile
        assert any(r[2] == H for r in multi) and any(r[2] == H and r[1] == 65 for r in rows)
    for flag in (4, 5, 6, 7):
        assert {r[flag] for r in multi} == {True, False}, flag
    assert {r[3] for r in multi} == {2, 3, 4}
    assert {(r[4], r[5]) for r in multi} == {(True, True), (True, False), (False, True), (False, False)}
    assert any(r[7] for r in multi if r[2] == 650) and any(r[7] for r in multi if r[2] < 650)
    assert 1 - np.float32(R.KEEP_H) == np.float32(0.25) and 1 - np.float32(R.KEEP_C) == np.float32(0.5)


@pytest.mark.parametrize('row', R.FS_CASES, ids=IDS)
def test_fp32_run_of_the_reference_stays_within_a_quarter_of_the_bar(row):
    case, r64, r32 = _refs(row)
    for name, bar in R.QUANTITIES:
        if r64[name] is None:
            continue
        assert torch.isfinite(r64[name]).all() and r64[name].abs().max() > 0, name
        e = R.margin_ok(name, r32[name], r64[name], bar)
        print('MARGIN %s %-7s fp32-cpu %.2e  bar %.0e' % (R.case_id(row), name, e, bar))


def test_inputs_can_see_a_wrong_kernel():
    """Mistakes a cell-step kernel can make, made on the inputs of the reference: each moves a checked quantity by more than 100 bars."""
    for row in ((5, 65, 9, 4, False, True, True, True), (2, 3, 650, 2, True, True, True, False)):
        case, r64, _ = _refs(row)
        T, B, H, L, masks, drop, last = row[:7]
        args = lambda **kw: {**dict(xg=case['xg'], W=case['W'], state=case['state'], mh=case['mh'] if masks else R.KEEP_H, mc=case['mc'] if masks else R.KEEP_C,
                                    dm=case['dm'], L=L, dy=case['dy'], d_last=case['d_last']), **kw}
        worst = {}
        W = [tuple(w.clone() for w in cell) for cell in case['W']]
        W[L][0][:, H - 1] = 0
        worst['last k of the slow cell\'s x W_ih^T dropped'] = R.fs_window_ref(**args(W=W))
        worst['dropout masks ignored'] = R.fs_window_ref(**args(dm=None))
        worst['zoneout ignored'] = R.fs_window_ref(**args(mh=1.0, mc=1.0))
        worst['final-state gradient ignored'] = R.fs_window_ref(**args(d_last=None))
        worst['zero initial state'] = R.fs_window_ref(**args(state=tuple(torch.zeros(B, H) for _ in range(4))))
        for what, wrong in worst.items():
            names = [n for n, _ in R.QUANTITIES if wrong[n] is not None and r64[n] is not None]
            bars = max(R.rel_err(wrong[n], r64[n]) / dict(R.QUANTITIES)[n] for n in names)
            print('SENSITIVITY %s %-44s %.1f bars' % (R.case_id(row), what, bars))
            assert bars > 100.0, (row, what, bars)


def test_cases_are_closed_under_the_plans():
    """No device is touched (cus = 256): every case's plans are the declared forms, every form a plan names over a sweep of shapes is
    declared and has a case, the plan's grid covers the shape with the tile it names, and a window is cells x T launches."""
    from robust_e2e_gan_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    declared = set()
    for T, B, H, L in (r[:4] for r in R.FS_CASES):
        for backward in (False, True):
            declared.add(R.plan_key(lib.fsrnn_plan(T, B, H, L, backward=backward, cus=256)))
    assert declared == set(R.FS_PLANS)
    named = set()
    for B in (1, 3, 64, 65, 256, 2048):
        for H in (1, 9, 33, 66, 512, 650, 1024):
            for T, L in ((1, 2), (35, 2), (5, 4)):
                for backward in (False, True):
                    p = lib.fsrnn_plan(T, B, H, L, backward=backward, cus=256)
                    named.add(R.plan_key(p))
                    gx, gy, gz = (int(v) for v in p['grid'].split('x'))
                    assert gz == 1 and gx * int(p['units']) >= H > (gx - 1) * int(p['units']) and gy * int(p['rows']) >= B > (gy - 1) * int(p['rows']), p
                    assert p['mfma'] == '16x16x4' and int(p['acc']) >= 2 and int(p['cells']) == L + 1 and int(p['launches']) == T * (L + 1), p
                    assert 0 < int(p['lds']) <= 65536, p
    assert named == declared
    for bad in ((0, 3, 8, 2), (4, 3, 8, 1), (35, 65536, 4096, 2)):          # no steps, one fast layer, gates beyond 32-bit element offsets
        with pytest.raises(lib.Re2eError):
            lib.fsrnn_plan(*bad, cus=256)
    so = lib.load()
    assert so.re2e_fsrnn_workspace_bytes(3, 650) >= 4 * 3 * 650 * 4


def test_model_refuses_what_the_reference_cannot_run():
    """fsrnn.py:118: fast_cells[1] is always run, on the slow cell's output -- S != F and fast_layers = 1 are refused, naming the line."""
    from robust_e2e_gan_amd.lib import Re2eError
    from robust_e2e_gan_amd.model.fsrnn import FSRNNLM
    with pytest.raises(Re2eError, match='fsrnn.py:118'):
        FSRNNLM(12, 6, 2, 10, 8, 0.9, 0.5)
    with pytest.raises(Re2eError, match='fsrnn.py:118'):
        FSRNNLM(12, 6, 1, 10, 10, 0.9, 0.5)
    m = FSRNNLM(12, 6, 3, 10, 10, 0.9, 0.5)
    assert ['predictor.' + k for k in m.state_dict()] == ['predictor.' + k for k in R.param_names(3)]
    assert all(float(p.detach().abs().max()) <= 0.1 for p in m.parameters())
    with pytest.raises(Re2eError):          # no CPU path
        m(None, torch.zeros(3, dtype=torch.long))


@pytest.mark.parametrize('L', (2, 3))
def test_reference_checkpoint_loads_strictly(golden_dir, L):
    from robust_e2e_gan_amd.model.fsrnn import FSRNNLM
    from robust_e2e_gan_amd.model.lm import ClassifierWithState
    fx = dict(np.load(os.path.join(golden_dir, 'fsrnn_tiny.npz')))
    pre = 'L%d.lm.' % L
    sd = {k[len(pre):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(pre)}
    m = ClassifierWithState(FSRNNLM(12, 6, L, 10, 10, 0.9, 0.5))
    m.load_state_dict(sd, strict=True)
    assert set(m.state_dict()) == set(sd)


def test_lm_train_dispatches_the_fsrnnlm(tmp_path, monkeypatch):
    """lm_train.main hands --lm-type fsrnnlm to model/fsrnn.py train with the FS-RNN arguments; model/lm.py train keeps refusing it; the FS-RNN
    trainer refuses training on the CPU before it opens a file."""
    from robust_e2e_gan_amd import lm_train
    from robust_e2e_gan_amd.lib import Re2eError
    from robust_e2e_gan_amd.model import fsrnn
    d = tmp_path / 'dict.txt'
    d.write_text(''.join('%d %d\n' % (i, i) for i in range(1, 10)))
    seen = {}
    monkeypatch.setattr(fsrnn, 'train', lambda args: seen.update(vars(args)) or 'trained')
    out = lm_train.main(['--ngpu', '1', '--outdir', str(tmp_path), '--dict', str(d), '--train-label', 'x', '--valid-label', 'y', '--lm-type', 'fsrnnlm',
                         '--fast_layers', '3', '--fast_cell_size', '10', '--slow_cell_size', '10', '--zoneout_keep_h', '0.75', '--zoneout_keep_c', '0.5'])
    assert out == 'trained' and seen['n_vocab'] == 11
    assert (seen['fast_layers'], seen['fast_cell_size'], seen['slow_cell_size'], seen['zoneout_keep_h'], seen['zoneout_keep_c']) == (3, 10, 10, 0.75, 0.5)
    monkeypatch.undo()
    args = argparse.Namespace(ngpu=0, lm_type='fsrnnlm', outdir='/nonexistent', train_label='/nonexistent/t', valid_label='/nonexistent/v')
    with pytest.raises(Re2eError):
        fsrnn.train(args)
    args.lm_type, args.ngpu = 'rnnlm', 1
    with pytest.raises(Re2eError):
        fsrnn.train(args)
