"""Pins tests/refs64_rnn.py (CPU only): the float64 recurrence reference against a packed bidirectional ``nn.LSTM`` in double; for every input
of tests/test_recurrence_kernels_gpu.py, that torch's own fp32 run of the reference stays within a quarter of the bar the HIP kernels are held
to there, and that the input can SEE a wrong kernel (five deliberate mistakes in the reference each move a checked quantity by more than a
hundred bars); and that ``RNN_CASES`` names exactly the kernel forms the launch plans of csrc/lstm.hip can name on a 256-CU chip."""
import functools
import itertools
import os

import pytest
import torch

import refs64_rnn as R
from test_abi import _LSTM_BUILT

IDS = [R.case_id(row) for row in R.RNN_CASES]


@functools.lru_cache(maxsize=None)
def _refs(B, H, T):
    case = R.rnn_case(B, T, H, seed=1000 * B + H + T)
    return case, R.case_ref(case), R.case_ref(case, torch.float32)


def _shapes():
    seen = []
    for row in R.RNN_CASES:
        if row[:3] not in seen:
            seen.append(row[:3])
    return seen


def test_table_case_is_a_function_of_the_shape():
    row = R.RNN_CASES[1]
    a, (b, _, _) = R.table_case(row), _refs(*row[:3])
    assert all(torch.equal(a[k], b[k]) for k in ('xg_f', 'xg_r', 'whh_f', 'whh_r', 'dy')) and a['lens'] == b['lens']
    assert len(set(IDS)) == len(IDS)


def test_reference_reproduces_packed_bidirectional_nn_lstm_in_double():
    """y, and through autograd dx, dW_hh and both bias gradients of each direction, on a ragged batch with a length-1 utterance; then what
    lstm_seq_ref derives by itself (d(gates), dbias) against the same run."""
    B, T, I, H = 5, 9, 11, 12
    lens = [9, 6, 6, 2, 1]
    g = torch.Generator().manual_seed(3)
    lstm = torch.nn.LSTM(I, H, 1, batch_first=False, bidirectional=True).double()
    for p in lstm.parameters():
        p.data = R.rnd(g, *p.shape, scale=0.4).double()
    x = R.rnd(g, T, B, I).double()
    dy = R.rnd(g, T, B, 2 * H, scale=0.3).double()          # values in the padded rows too
    valid = R.valid_mask(lens, T).unsqueeze(2)
    xr = x.clone().requires_grad_(True)
    pk = torch.nn.utils.rnn.pack_padded_sequence(xr, torch.tensor(lens))
    yr, _ = torch.nn.utils.rnn.pad_packed_sequence(lstm(pk)[0], total_length=T)
    (yr * dy).sum().backward()
    want = {n: getattr(lstm, n).grad.clone() for n, _ in lstm.named_parameters()}
    # the same through the reference's core, from leaves of its own
    P = {n: p.detach().clone().requires_grad_(True) for n, p in lstm.named_parameters()}
    xm = x.clone().requires_grad_(True)
    xg = [xm @ P['weight_ih_l0' + s].t() + P['bias_ih_l0' + s] + P['bias_hh_l0' + s] for s in ('', '_reverse')]
    xg = [torch.where(valid, v, torch.full_like(v, float('nan'))) for v in xg]          # never read beyond the lengths
    y, c, gf, gr, _ = R.lstm_seq_forward(xg[0], xg[1], P['weight_hh_l0'], P['weight_hh_l0_reverse'], lens)
    (y * dy).sum().backward()
    assert R.rel_err(y, yr) <= 1e-12
    assert (y[~valid.expand_as(y)] == 0).all() and (c[~valid.expand_as(c)] == 0).all()
    assert R.rel_err(xm.grad, xr.grad) <= 1e-12
    for n in want:
        assert R.rel_err(P[n].grad, want[n]) <= 1e-12, n
    # lstm_seq_ref: its d(gates) give the same dx and bias gradients, its dbias is their column sum
    with torch.no_grad():
        xg0 = [x @ P['weight_ih_l0' + s].t() + P['bias_ih_l0' + s] + P['bias_hh_l0' + s] for s in ('', '_reverse')]
        xg0 = [torch.where(valid, v, torch.full_like(v, float('nan'))) for v in xg0]
    r = R.lstm_seq_ref(xg0[0], xg0[1], P['weight_hh_l0'], P['weight_hh_l0_reverse'], lens, dy)
    assert R.rel_err(r['y'], yr) <= 1e-12
    dx = r['dgates_f'] @ P['weight_ih_l0'].detach() + r['dgates_r'] @ P['weight_ih_l0_reverse'].detach()
    assert R.rel_err(dx, xr.grad) <= 1e-12
    for d, s in enumerate(('', '_reverse')):
        assert R.rel_err(r['dbias'][d], want['bias_ih_l0' + s]) <= 1e-12 and R.rel_err(r['dbias'][d], want['bias_hh_l0' + s]) <= 1e-12
        dg = r['dgates_r' if d else 'dgates_f']
        assert (dg[~valid.expand_as(dg)] == 0).all()
        # dW_hh = sum_t d(gates)_t^T h_(previous step): the outputs are zero beyond the lengths, which is the reverse direction's start state
        hprev = torch.zeros(T, B, H, dtype=torch.float64)
        if d:
            hprev[:-1] = r['y'][1:, :, H:]
        else:
            hprev[1:] = r['y'][:-1, :, :H]
        assert R.rel_err(dg.reshape(T * B, 4 * H).t() @ hprev.reshape(T * B, H), want['weight_hh_l0' + s]) <= 1e-12
    for k, v in r.items():
        assert torch.isfinite(v).all(), k


@pytest.mark.parametrize('B,H,T', _shapes())
def test_fp32_run_of_the_reference_stays_within_a_quarter_of_the_bar(B, H, T):
    case, r64, r32 = _refs(B, H, T)
    assert case['lens'][0] == T and case['lens'][-1] == 1 and min(case['lens']) < T
    for name, bar in R.QUANTITIES:
        assert torch.isfinite(r64[name]).all(), name
        e = R.margin_ok(name, r32[name], r64[name], bar)
        print('MARGIN B%d-H%d-T%d %-9s fp32-cpu %.2e  bar %.0e' % (B, H, T, name, e, bar))


@pytest.mark.parametrize('B,H,T', _shapes())
def test_inputs_can_see_a_wrong_kernel(B, H, T):
    """Each mistake, made in the reference, moves at least one checked quantity by more than 100 bars on this input."""
    case, r64, _ = _refs(B, H, T)
    for m, what in R.MISTAKES.items():
        wrong = R.case_ref(case, mistake=m)
        worst = max(R.rel_err(wrong[name], r64[name]) / bar for name, bar in R.QUANTITIES)
        print('SENSITIVITY B%d-H%d-T%d (%s) %-62s %.1f bars' % (B, H, T, m, what, worst))
        assert worst > 100.0, 'mistake (%s) %s moves nothing by more than %.1f bars at B=%d H=%d T=%d' % (m, what, worst, B, H, T)


# Instantiations no plan names on a 256-CU chip under any value of the five switches (B <= 300, H <= 1024): input for a later clean-up.
# lstm_fwd2 takes a layer narrower than 384 only at one utterance tile, where the smallest tile count whose grid fits half of the chip is
# fixed by H alone (1 up to H = 256, 2 at H = 320), and at H = 512 one tile per workgroup never fits; lstm_bwd3 runs 8 units per workgroup
# only while H / 8 workgroups per utterance tile and direction fit a quarter of the chip, which ends at H = 256.
NEVER_NAMED_ON_256 = sorted(
    [('bwd3', 8, t) for t in (5, 6, 7, 8)] +
    [(fam, tl, nj) for fam in ('fwd2_persist', 'fwd2_step') for tl, nj in ((1, 5), (1, 8), (2, 1), (2, 2), (2, 4), (4, 1), (4, 2), (4, 4), (4, 5))])

_SWEEP_B = (1, 3, 8, 16, 17, 24, 32, 33, 40, 64, 65, 70, 96, 128, 129, 160, 256, 300)


def _set_switches(monkeypatch, env):
    for k in R.RNN_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        if v is not None:
            monkeypatch.setenv(k, v)


def test_cases_are_closed_under_the_plans(monkeypatch):
    """No device is touched (cus = 256).  (i) every (family, a, b) a plan names over the sweep has a row in RNN_CASES and the other way
    round; (ii) what is built and never named is NEVER_NAMED_ON_256, literally; and every row's declared plans are what the library answers."""
    from robust_e2e_gan_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    named = set()
    values = {R.RNN_SWITCHES[0]: (None, '0'), R.RNN_SWITCHES[1]: (None, '0'), R.RNN_SWITCHES[2]: (None, '0'), R.RNN_SWITCHES[3]: (None, '0'),
              R.RNN_SWITCHES[4]: (None, '1', '2')}
    for combo in itertools.product(*(values[k] for k in R.RNN_SWITCHES)):
        _set_switches(monkeypatch, dict(zip(R.RNN_SWITCHES, combo)))
        for B in _SWEEP_B:
            for H in range(8, 1025, 8):
                for backward in (False, True):
                    named.add(R.plan_key(lib.lstm_plan(7, B, H, backward=backward, cus=256)))
    declared = set()
    for B, H, T, env, fwd, bwd in R.RNN_CASES:
        _set_switches(monkeypatch, env)
        assert R.plan_key(lib.lstm_plan(T, B, H, cus=256)) == fwd, (B, H, T, env)
        assert R.plan_key(lib.lstm_plan(T, B, H, backward=True, cus=256)) == bwd, (B, H, T, env)
        declared |= {fwd, bwd}
    assert named == declared, ('reachable without a numeric case', sorted(named - declared, key=str), 'declared and never named', sorted(declared - named, key=str))
    built = {(fam, a, b) for fam, (_, _, forms) in _LSTM_BUILT.items() for a, b in forms}
    assert named <= built
    assert sorted(built - named, key=str) == sorted(NEVER_NAMED_ON_256, key=str)
    assert len(built) == 68 and len(NEVER_NAMED_ON_256) == 22
