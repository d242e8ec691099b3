"""The recurrences of csrc/lstm.hip against the float64 reference of tests/refs64_rnn.py, through the C ABI (re2e_lstm_seq_fwd / _bwd), one row
per kernel form the launch plans can name on a 256-CU chip: every row of refs64_rnn.RNN_CASES first asserts that the library's plan for its
shape and switches IS the form the row declares, so a routing change cannot quietly empty a row (tests/test_refs64_rnn_cpu.py checks that
the table is closed under the plans).  A second test turns the edges the table does not: one and two steps, every length 1 / T, batch
sizes at both sides of the 16- and 32-utterance tiles under each family, a W_hh that is not 16-byte aligned, no bias gradient.

Every call: pre-activations beyond each length are NaN (they are never to be read), the workspace is NaN, forward and backward run twice
on fresh copies (stale tags of the first call must not satisfy the second), dy carries values in the padded rows.  Checked against float64:
y, c and the activated gates over the valid rows, d(gates) and dbias everywhere, exact zeros beyond the lengths, untouched border blocks,
no give-up.  The bars are the project's own (test_bilstm): 1e-4 of the tensor's max for outputs, 2e-4 for gradients; each quantity first
asserts that torch's fp32 CPU run of the reference stays within a quarter of its bar, then prints both distances.  GPU only.

Measured on an MI355X when the module was written, worst case per kernel family and quantity, HIP / fp32 on the CPU (of the tensor's max):
    fwd_step:     y 2.3e-7 / 2.0e-7, c 1.8e-7 / 1.7e-7, gates 4.9e-7 / 2.9e-7 (H = 392, one wavefront over all of K)
    fwd_persist:  y 2.3e-7 / 2.8e-7, c 1.7e-7 / 1.6e-7, gates 1.7e-7 / 3.6e-7
    fwd2_persist: y 2.1e-7 / 2.1e-7, c 1.4e-7 / 1.5e-7, gates 2.4e-7 / 3.0e-7
    fwd2_step:    y 1.9e-7 / 2.2e-7, c 1.6e-7 / 1.5e-7, gates 4.3e-7 / 3.5e-7      (bar 1e-4 for all of these)
    bwd3:         d(gates) 2.2e-7 / 4.0e-7, dbias 2.2e-7 / 3.0e-7
    bwd_persist:  d(gates) 2.8e-7 / 3.4e-7, dbias 2.2e-7 / 5.4e-7
    bwd_step:     d(gates) 2.3e-7 / 3.3e-7, dbias 3.6e-7 / 2.5e-7 (B = 300)          (bar 2e-4)
    W_hh off 16-byte alignment (H = 64, 512): y 1.8e-7, c 1.5e-7, gates 1.5e-7
Every form is where fp32 arithmetic puts it: three orders inside the bars, no row or edge stands out."""
import functools

import pytest
import torch

import refs64_rnn as R
from test_loss_kernels_gpu import DEV, _held, _ops

pytestmark = pytest.mark.gpu

NAN = float('nan')


@functools.lru_cache(maxsize=None)
def _table_refs(B, H, T):
    case = R.table_case((B, H, T))
    return case, R.case_ref(case), R.case_ref(case, torch.float32)


def _set_switches(monkeypatch, env):
    for k in R.RNN_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _run_hip(lib, case, misalign=False, dbias=True):
    """re2e_lstm_seq_fwd twice, then re2e_lstm_seq_bwd twice from the second forward's state -> dict of CPU tensors (the names of lstm_seq_ref, plus
    the border blocks of ybuf / cbuf)."""
    T, B, H = case['T'], case['B'], case['H']
    pad = ~R.valid_mask(case['lens'], T)
    xg0 = []
    for k in ('xg_f', 'xg_r'):
        v = case[k].clone()
        v[pad] = NAN                                                           # never read: whatever they hold must not matter
        xg0.append(v.reshape(T * B, 4 * H).to(DEV))
    if misalign:                                                              # 4 bytes off a 16-byte boundary
        store = [torch.empty(4 * H * H + 4, device=DEV) for _ in range(2)]
        whh = [s[1:1 + 4 * H * H].view(4 * H, H) for s in store]
        for w, k in zip(whh, ('whh_f', 'whh_r')):
            w.copy_(case[k])
            assert w.data_ptr() % 16 == 4
    else:
        whh = [case[k].to(DEV) for k in ('whh_f', 'whh_r')]
        assert all(w.data_ptr() % 16 == 0 for w in whh)
    lens = torch.tensor(case['lens'], dtype=torch.int32, device=DEV)
    dy = case['dy'].reshape(T * B, 2 * H).to(DEV)
    wsb = lib.query('re2e_lstm_workspace_bytes', B, H)
    ws = torch.full((wsb // 4 + 16,), NAN, device=DEV)                        # poisoned: nothing may be read before it is written
    xg = [x.clone() for x in xg0]
    ybuf, cbuf = torch.zeros(T + 2, B, 2 * H, device=DEV), torch.zeros(T + 2, B, 2 * H, device=DEV)
    for _ in range(2):
        for d in range(2):
            xg[d].copy_(xg0[d])
        ybuf[1:T + 1].fill_(NAN)                                              # every block between the borders is the call's to write
        cbuf[1:T + 1].fill_(NAN)
        lib.call('re2e_lstm_seq_fwd', xg[0].data_ptr(), xg[1].data_ptr(), whh[0].data_ptr(), whh[1].data_ptr(), ybuf.data_ptr(), cbuf.data_ptr(),
                 lens.data_ptr(), T, B, H, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    ws = torch.full((wsb // 4 + 16,), NAN, device=DEV)
    db = torch.full((2, 4 * H), NAN, device=DEV) if dbias else None
    for _ in range(2):
        G = [x.clone() for x in xg]
        dc = torch.full((B, 2 * H), NAN, device=DEV)
        if db is not None:
            db.fill_(NAN)
        lib.call('re2e_lstm_seq_bwd', G[0].data_ptr(), G[1].data_ptr(), whh[0].data_ptr(), whh[1].data_ptr(), dy.data_ptr(), ybuf.data_ptr(),
                 cbuf.data_ptr(), dc.data_ptr(), lens.data_ptr(), T, B, H, db.data_ptr() if db is not None else None, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    cpu = lambda v, w: v.cpu().view(T, B, w)
    return dict(y=ybuf[1:T + 1].cpu(), c=cbuf[1:T + 1].cpu(), gates_f=cpu(xg[0], 4 * H), gates_r=cpu(xg[1], 4 * H), dgates_f=cpu(G[0], 4 * H),
                dgates_r=cpu(G[1], 4 * H), dbias=db.cpu() if db is not None else None,
                borders=torch.stack([ybuf[0], ybuf[T + 1], cbuf[0], cbuf[T + 1]]).cpu())


def _check(tag, case, got, r64, r32):
    T = case['T']
    valid = R.valid_mask(case['lens'], T)
    assert (got['borders'] == 0).all(), 'border blocks 0 and T + 1 of ybuf / cbuf must stay zero'
    for name, bar in R.QUANTITIES:
        if got[name] is None:
            continue
        g, f64, f32 = got[name], r64[name], r32[name]
        if name.startswith('gates'):                       # the activated gates of a padded frame are nobody's to read
            g, f64, f32 = g[valid], f64[valid], f32[valid]
        assert torch.isfinite(g).all(), '%s %s: not finite where the reference is' % (tag, name)
        _held(tag, name, g, f64, f32, bar)
    for name in ('y', 'c', 'dgates_f', 'dgates_r'):
        assert (got[name][~valid] == 0).all(), '%s %s: frames at or beyond the lengths must be exact zeros' % (tag, name)
        assert got[name][valid].abs().max() > 0


@pytest.mark.parametrize('row', R.RNN_CASES, ids=R.case_id)
def test_recurrence_against_float64(row, monkeypatch):
    ops, lib = _ops()
    B, H, T, env, fwd, bwd = row
    _set_switches(monkeypatch, env)
    assert R.plan_key(lib.lstm_plan(T, B, H)) == fwd, lib.lstm_plan(T, B, H)
    assert R.plan_key(lib.lstm_plan(T, B, H, backward=True)) == bwd, lib.lstm_plan(T, B, H, backward=True)
    case, r64, r32 = _table_refs(B, H, T)
    aborts = lib.query('re2e_lstm_abort_count')          # (per process: tests of the give-up protocol before this one leave it above zero)
    got = _run_hip(lib, case)
    _check('%s %s%s %s%s' % (R.case_id(row), fwd[0], fwd[1:], bwd[0], bwd[1:]), case, got, r64, r32)
    assert lib.query('re2e_lstm_abort_count') == aborts, 'a persistent recurrence gave up on a peer workgroup'


_NO_PERSIST = {'RE2E_LSTM_PERSIST': '0', 'RE2E_LSTM_PERSIST_BWD': '0'}          # fwd2_step (<= 16 utterances) / fwd_step, bwd_step
_ROUND_1_3 = {'RE2E_LSTM_FWD2': '0', 'RE2E_LSTM_BWD3': '0'}                      # fwd_persist, bwd_persist
# (name, B, H, T, lens (None: rnn_lens; an int: every length), switches, misaligned W_hh, dbias requested)
EDGES = (
    [('one-step', B, H, 1, None, {}, False, True) for B, H in ((3, 64), (17, 256))] +          # T = 1: the launch-per-step forms
    [('two-steps', B, H, 2, None, {}, False, True) for B, H in ((3, 64), (17, 256), (3, 144))] +
    [('every-length-1', B, H, 7, 1, {}, False, True) for B, H in ((3, 64), (17, 256), (3, 144))] +
    [('every-length-T', B, H, 7, 7, {}, False, True) for B, H in ((3, 64), (17, 256), (3, 144))] +
    # both sides of the 16- and 32-utterance tiles, under each family: fwd2_persist / fwd_persist(4,2) + bwd3; the launch-per-step forms;
    # fwd_persist + bwd_persist
    [('tile-edge', B, 64, 7, None, env, False, True) for env in ({}, _NO_PERSIST, _ROUND_1_3) for B in (15, 16, 17, 31, 32, 33)] +
    # plan_fwd must decline lstm_fwd2 (it reads W_hh in 16-byte pieces) and the result must still be right
    [('misaligned-whh', B, H, 7, None, {}, True, True) for B, H in ((3, 64), (3, 512))] +
    # dbias = NULL must not disturb d(gates): beside the recurrence (bwd3) and behind it (bwd_persist)
    [('no-dbias', B, H, 7, None, {}, False, False) for B, H in ((3, 64), (3, 144))])


def _edge_id(e):
    name, B, H, T, lens, env, misalign, dbias = e
    return '%s-B%d-H%d-T%d%s' % (name, B, H, T, ''.join('-%s=%s' % (k[len('RE2E_LSTM_'):], v) for k, v in sorted(env.items())))


@functools.lru_cache(maxsize=None)
def _edge_refs(B, H, T, lens):
    case = R.rnn_case(B, T, H, seed=7000 + 1000 * B + H + T, lens=None if lens is None else [lens] * B)
    return case, R.case_ref(case), R.case_ref(case, torch.float32)


@pytest.mark.parametrize('edge', EDGES, ids=_edge_id)
def test_recurrence_edges_against_float64(edge, monkeypatch):
    ops, lib = _ops()
    name, B, H, T, lens, env, misalign, dbias = edge
    _set_switches(monkeypatch, env)
    fwd, bwd = R.plan_key(lib.lstm_plan(T, B, H)), R.plan_key(lib.lstm_plan(T, B, H, backward=True))
    if T == 1:
        assert fwd[0].endswith('_step') and bwd[0] == 'bwd_step', (fwd, bwd)
    case, r64, r32 = _edge_refs(B, H, T, lens)
    aborts = lib.query('re2e_lstm_abort_count')
    got = _run_hip(lib, case, misalign=misalign, dbias=dbias)
    # (the plan query assumes aligned weights: no forward plan to name for the misaligned call)
    _check('%s %s %s%s' % (_edge_id(edge), 'fwd-unaligned' if misalign else '%s%s' % (fwd[0], fwd[1:]), bwd[0], bwd[1:]), case, got, r64, r32)
    assert lib.query('re2e_lstm_abort_count') == aborts, 'a persistent recurrence gave up on a peer workgroup'
