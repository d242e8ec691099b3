"""The decode-time kernels -- the CTC prefix scorers of csrc/ctc.hip (re2e_ctc_prefix_score, _batch, _cands) and the few-row language-model
kernels of csrc/rnnlm.hip (re2e_lm_lstm_cell, re2e_lm_output, re2e_lm_log_softmax_combine, re2e_lm_add_cands) -- against the float64
references of tests/refs64_dec.py, through the C ABI, at the smallest shapes where they can go wrong (refs64_dec.PREFIX_CASES, LM_CELL_CASES,
LM_OUT_CASES, LSM_CASES).

Prefix scorers: every row of the table on each entry point it names, chained over four output positions.  The candidates of the top-k entry
points must be the first ctc_beam labels of a stable descending sort of the fp32 attention row, exactly; prefix scores, local scores and
the state rows the next position reads must be dead (<= -1e9), -inf or live exactly where float64 is, and live values within 2e-5 of the
largest live magnitude (the one row with its own bar for the states says why in the table).  The _batch rows are compared with float64
directly.  Every LM row first asserts that re2e_lm_plan, asked with the call's own pointers, names the kernel form the table declares, then
holds h and c to 1e-4 and the logits to 2e-4 of the tensor's max; log-softmax rows to 1e-4, the combined score bitwise to att + fl(w lsm)
from the kernel's own lsm; re2e_lm_add_cands bitwise to the fp32 gather-multiply-add.  Each comparison with float64 first asserts that the
fp32 CPU run of the same reference stays within a quarter of the bar, then prints both distances.  Output buffers start as NaN (integers
as -777) with a sentinel block behind them.  GPU only.

Measured on an MI355X when the module was written, worst case per quantity, HIP / fp32 on the CPU (numpy for the prefix scores, torch for the
rest), of the live max / of the tensor's max:
    prefix scores 6.2e-8 / 6.2e-8, local scores 1.4e-7 / 1.4e-7, states 8.0e-7 / 8.0e-7 (bar 2e-5; T = 257); the kernels' logaddexp is
    numpy's float32 one, term by term, and lands where numpy does.  States at T = 5400: 6.2e-5 / 6.2e-5 (that row's bar 3e-4)
    cell: h 2.9e-7 / 7.3e-7, c 1.7e-7 / 3.9e-7 (bar 1e-4); logits 1.3e-7 / 3.5e-7 (2e-4); log-softmax rows 6.7e-8 / 8.0e-8 (1e-4)
The module found one defect: comb and re2e_lm_add_cands rounded once, not twice -- __fadd_rn(a, __fmul_rn(w, x)) is a plain a + w * x to the
compiler, which contracted it into one FMA (rows V1024-n1 and every weighted row after it; fixed in csrc/rnnlm.hip, add_scaled).
"""
import numpy as np
import pytest
import torch

import refs64_dec as R
from test_loss_kernels_gpu import DEV, _held, _i32, _ops

pytestmark = pytest.mark.gpu

NAN = float('nan')
SENTINEL = 123.0


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _at(t, off_bytes=0):
    """A device copy of ``t`` that starts ``off_bytes`` past a 16-byte boundary."""
    store = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
    k = off_bytes // 4
    v = store[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off_bytes and v.is_contiguous()
    return v


def _p(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------
# prefix scorers
# ---------------------------------------------------------------------------------------------
def _held_live(case, name, got, f64, f32, bar, mask=None):
    """Classes first (dead / -inf / NaN exactly where float64 has them), then the precondition (fp32 CPU within a quarter of the bar) and the
    HIP result within the bar, both of the largest live magnitude; prints both distances."""
    sel = mask if mask is not None else np.ones(np.shape(f64), dtype=bool)
    cg, cr = R.classes(got), R.classes(f64)
    assert (cg == cr)[sel].all(), '%s %s: %d entries are dead / -inf / NaN where float64 is not, or the reverse' % (case, name, int((cg != cr)[sel].sum()))
    cpu = R.live_err(f32, f64, mask)
    assert cpu <= 0.25 * bar, 'input too hard for the bar: fp32 CPU reference of %s is %.3e from float64, the bar is %.1e' % (name, cpu, bar)
    err = R.live_err(got, f64, mask)
    print('ERR %-46s %-16s hip %.2e  fp32-cpu %.2e  bar %.0e' % (case, name, err, cpu, bar))
    assert err <= bar, '%s %s: HIP is %.3e of the live max from float64 (bar %.1e, fp32 on the CPU: %.3e)' % (case, name, err, bar, cpu)


def _run_prefix(lib, entry, L, cb):
    nh, Tmax, V, eos = len(L['olen']), L['Tmax'], L['V'], L['eos']
    nc = L['cands'].shape[1]
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    lpz = D(L['lpz'] if entry == 'batch' else L['lpz'][0])
    att, r_prev, prev = D(L['att']), D(L['r_prev']), D(L['prev'])
    last, olen = _i32(L['last']), _i32(L['olen'])
    cand = torch.full((nh, nc), -777, dtype=torch.int32, device=DEV)
    loc, psi = _nan(nh, nc), _nan(nh, nc)
    r_new = _nan(nh * nc + 1, Tmax, 2)
    r_new[nh * nc] = SENTINEL                                                    # one spare state block behind the last candidate
    common = (R.ATT_WEIGHT, R.CTC_WEIGHT, R.BLANK, eos)
    if entry == 'topk':
        lib.call('re2e_ctc_prefix_score', lpz.data_ptr(), Tmax, V, att.data_ptr(), nh, r_prev.data_ptr(), last.data_ptr(), olen.data_ptr(), prev.data_ptr(),
                 cb, *common, cand.data_ptr(), loc.data_ptr(), psi.data_ptr(), r_new.data_ptr())
    elif entry == 'batch':
        tl, utt = _i32(L['tlen']), _i32(L['utt'])
        lib.call('re2e_ctc_prefix_score_batch', lpz.data_ptr(), L['U'], Tmax, V, tl.data_ptr(), utt.data_ptr(), att.data_ptr(), nh, r_prev.data_ptr(),
                 last.data_ptr(), olen.data_ptr(), prev.data_ptr(), cb, *common, cand.data_ptr(), loc.data_ptr(), psi.data_ptr(), r_new.data_ptr())
    else:
        cin = _i32(L['cands'])
        lib.call('re2e_ctc_prefix_score_cands', lpz.data_ptr(), Tmax, V, att.data_ptr(), nh, r_prev.data_ptr(), last.data_ptr(), olen.data_ptr(),
                 prev.data_ptr(), cin.data_ptr(), nc, *common, loc.data_ptr(), psi.data_ptr(), r_new.data_ptr())
    torch.cuda.synchronize()
    assert bool((r_new[nh * nc] == SENTINEL).all()), 'state writes ran past the last candidate block'
    return cand.cpu().numpy(), loc.cpu().numpy(), psi.cpu().numpy(), r_new[:nh * nc].cpu().numpy().reshape(nh, nc, Tmax, 2)


@pytest.mark.parametrize('name,entry', [(c['name'], e) for c in R.PREFIX_CASES for e in c['entries']])
def test_prefix_scorers_against_float64(name, entry):
    ops, lib = _ops()
    case = R.PREFIX_CASES[R.PREFIX_IDS.index(name)]
    for pos, L in enumerate(R.prefix_chain(name, entry)):
        what = '%s-%s-pos%d' % (name, entry, pos)
        cand, loc, psi, r = _run_prefix(lib, entry, L, case['cb'])
        if entry != 'cands':
            assert cand.tolist() == L['cands'].tolist(), '%s: candidates differ from the stable descending sort of the attention row' % what
        else:
            assert (cand == -777).all()
        f64, f32 = L['f64'], L['f32']
        _held_live(what, 'ctc_score', psi, f64['psi'], f32['psi'], case['bar'])
        _held_live(what, 'local', loc, f64['local'], f32['local'], case['bar'])
        _held_live(what, 'r_new', r, f64['r'], f32['r'], case['bar_r'], R.read_mask(r.shape, L['starts']))
        for k in range(r.shape[0]):
            T = L['T'][int(L['utt'][k])]
            assert (r[k, :, T:] == np.float32(R.LOGZERO)).all(), '%s: state rows at t >= T_u are not dead' % what


def test_prefix_scorers_refuse():
    """ctc_beam 65; ctc_beam > V; V + 3T floats above 150 KB; more candidates than labels.  Nothing is launched: the operands are one small tensor."""
    ops, lib = _ops()
    z, zi = torch.zeros(4096, device=DEV), torch.zeros(4096, dtype=torch.int32, device=DEV)
    P, I = z.data_ptr(), zi.data_ptr()

    def topk(T, V, cb):
        lib.call('re2e_ctc_prefix_score', P, T, V, P, 1, P, I, I, P, cb, 0.7, 0.3, 0, V - 1, I, P, P, P)

    def batch(T, V, cb):
        lib.call('re2e_ctc_prefix_score_batch', P, 1, T, V, I, I, P, 1, P, I, I, P, cb, 0.7, 0.3, 0, V - 1, I, P, P, P)

    def cands(T, V, nc):
        lib.call('re2e_ctc_prefix_score_cands', P, T, V, P, 1, P, I, I, P, I, nc, 0.7, 0.3, 0, V - 1, P, P, P)

    for f, args in ((topk, (9, 100, 65)), (batch, (9, 100, 65)), (topk, (9, 5, 6)), (batch, (9, 5, 6)), (topk, (12800, 23, 4)), (batch, (12800, 23, 4)),
                    (cands, (12801, 23, 4)), (cands, (9, 5, 6))):
        with pytest.raises(lib.Re2eError):
            f(*args)
    assert bool((z == 0).all()) and bool((zi == 0).all())


# ---------------------------------------------------------------------------------------------
# the LSTM cell and the output layer
# ---------------------------------------------------------------------------------------------
def _cell_call(lib, row, d, ids=None, entry='re2e_lm_lstm_cell'):
    """-> h, c (n,H) on the CPU; the plan the library names for exactly these operands is asserted first."""
    n, I, H, ldx = row['n'], row['I'], row['H'], row['ldx']
    off = lambda k: row['off'].get(k, 0)
    x = _at(d['xfull'], off('x'))
    w_ih, w_hh, b_ih, b_hh = _at(d['w_ih'], off('w_ih')), _at(d['w_hh'], off('w_hh')), _at(d['b_ih']), _at(d['b_hh'])
    hp = _at(d['h_prev'], off('h_prev')) if d['h_prev'] is not None else None
    cp = _at(d['c_prev']) if d['c_prev'] is not None else None
    ids = d['ids'] if ids is None else ids
    ids_d = _i32(ids) if ids is not None else None
    plan = lib.lm_plan(lib.LM_PLAN_CELL, x=x.data_ptr(), ldx=ldx, I=I, w_ih=w_ih.data_ptr(), w_hh=w_hh.data_ptr(), h_prev=_p(hp), n=n, H=H)
    assert (plan['family'], int(plan['rows']), int(plan['vi']), int(plan['vh'])) == ('lm_cell',) + row['form'], (row['name'], plan)
    assert plan['grid'] == '%dx1x1' % H and int(plan['trips']) == -(-n // row['form'][0]), (row['name'], plan)
    out = _nan(2, n * H + 64)
    out[:, n * H:] = SENTINEL
    lib.call(entry, x.data_ptr(), ldx, _p(ids_d), d['xfull'].shape[0] if ids is not None else 0, I, w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(),
             b_hh.data_ptr(), _p(hp), _p(cp), n, H, out[0].data_ptr(), out[1].data_ptr())
    torch.cuda.synchronize()
    assert bool((out[:, n * H:] == SENTINEL).all()), 'written beyond the (n, H) outputs'
    return out[0, :n * H].view(n, H).cpu(), out[1, :n * H].view(n, H).cpu()


@pytest.mark.parametrize('row', R.LM_CELL_CASES, ids=[r['name'] for r in R.LM_CELL_CASES])
def test_lm_lstm_cell_against_float64(row):
    ops, lib = _ops()
    d = R.cell_inputs(row)
    h, c = _cell_call(lib, row, d)
    (h64, c64), (h32, c32) = R.cell_case_ref(d), R.cell_case_ref(d, torch.float32)
    assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(c).all()), row['name']
    _held(row['name'], 'h', h, h64, h32, R.BAR_OUT)
    _held(row['name'], 'c', c, c64, c32, R.BAR_OUT)


@pytest.mark.parametrize('name', ['I8-H10-n9', 'I8-H12-n17', 'recipe-l1'])
def test_lm_lstm_cell_poisons_bad_ids(name):
    """An id of -1 or n_embed gives a NaN row of h and c -- never a read outside the table -- and leaves every other row within the bar."""
    ops, lib = _ops()
    row = dict(next(r for r in R.LM_CELL_CASES if r['name'] == name), x='ids')
    d = R.cell_inputs(row)
    n, nrow = row['n'], d['xfull'].shape[0]
    ids = d['ids'].clone()
    bad = [1, n - 2]
    ids[bad[0]], ids[bad[1]] = -1, nrow
    good = [r for r in range(n) if r not in bad]
    h, c = _cell_call(lib, row, d, ids=ids)
    assert bool(torch.isnan(h[bad]).all()) and bool(torch.isnan(c[bad]).all())
    assert bool(torch.isfinite(h[good]).all()) and bool(torch.isfinite(c[good]).all())
    (h64, c64), (h32, c32) = R.cell_case_ref(d), R.cell_case_ref(d, torch.float32)
    _held(name + '-bad-ids', 'h', h[good], h64[good], h32[good], R.BAR_OUT)
    _held(name + '-bad-ids', 'c', c[good], c64[good], c32[good], R.BAR_OUT)


def test_lm_lstm_cell_refuses():
    """n = 0 and n = 65; an output that aliases h_prev; rows of x shorter than I; ids without a table.  Nothing is launched."""
    ops, lib = _ops()
    n, I, H = 4, 8, 12
    z = torch.zeros(65 * 4 * H * I, device=DEV)
    o1, o2, hp = _nan(65 * H), _nan(65 * H), torch.zeros(65 * H, device=DEV)
    zi = torch.zeros(65, dtype=torch.int32, device=DEV)
    P = z.data_ptr()

    def call(x=P, ldx=I, ids=None, n_embed=0, n=n, h_prev=hp.data_ptr(), h_out=o1.data_ptr(), c_out=o2.data_ptr()):
        lib.call('re2e_lm_lstm_cell', x, ldx, ids, n_embed, I, P, P, P, P, h_prev, hp.data_ptr(), n, H, h_out, c_out)

    call()                                                                       # the supported call, for contrast
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o1[:n * H]).all()) and bool(torch.isnan(o1[n * H:]).all())
    o1.fill_(NAN)
    for bad in (dict(n=0), dict(n=65), dict(h_out=hp.data_ptr()), dict(c_out=hp.data_ptr()), dict(ldx=I - 1), dict(x=None, ids=zi.data_ptr(), n_embed=4)):
        with pytest.raises(lib.Re2eError):
            call(**bad)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o1).all()) and bool(torch.isnan(o2[n * H:]).all()) and bool((hp == 0).all())


@pytest.mark.parametrize('row', R.LM_OUT_CASES, ids=[r['name'] for r in R.LM_OUT_CASES])
def test_lm_output_against_float64(row):
    ops, lib = _ops()
    n, V, H = row['n'], row['V'], row['H']
    d = R.out_inputs(row)
    h, w, b = _at(d['h'], row['off'].get('h', 0)), _at(d['w'], row['off'].get('w', 0)), _at(d['b'])
    plan = lib.lm_plan(lib.LM_PLAN_OUTPUT, w_hh=w.data_ptr(), h_prev=h.data_ptr(), n=n, H=H, V=V)
    assert (plan['family'], int(plan['rows']), int(plan['vec'])) == ('lm_out',) + row['form'], (row['name'], plan)
    assert plan['grid'] == '%dx1x1' % ((V + 3) // 4), (row['name'], plan)
    out = _nan(n * V + 64)
    out[n * V:] = SENTINEL
    lib.call('re2e_lm_output', h.data_ptr(), w.data_ptr(), b.data_ptr(), n, V, H, out.data_ptr())
    torch.cuda.synchronize()
    assert bool((out[n * V:] == SENTINEL).all()), 'written beyond the (n, V) logits'
    got = out[:n * V].view(n, V).cpu()
    assert bool(torch.isfinite(got).all()), row['name']
    _held(row['name'], 'logits', got, R.out_ref(d['h'], d['w'], d['b']), R.out_ref(d['h'], d['w'], d['b'], torch.float32), R.BAR_LOGITS)


def test_lm_output_refuses():
    ops, lib = _ops()
    z, o = torch.zeros(65 * 12, device=DEV), _nan(65 * 5)
    for n in (0, 65):
        with pytest.raises(lib.Re2eError):
            lib.call('re2e_lm_output', z.data_ptr(), z.data_ptr(), z.data_ptr(), n, 5, 12, o.data_ptr())
    assert bool(torch.isnan(o).all())


# ---------------------------------------------------------------------------------------------
# log-softmax (+ the combined score), candidates' LM scores
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V,n', R.LSM_CASES)
def test_lm_log_softmax_combine_against_float64(V, n):
    ops, lib = _ops()
    d = R.lsm_inputs(V, n)
    x, att, w = d['logits'].to(DEV), d['att'].to(DEV), d['lm_weight']
    l64, l32 = R.lsm_ref(d['logits']), R.lsm_ref(d['logits'], torch.float32)
    alone = None
    for with_att in (False, True):
        lsm, comb = _nan(n * V + 64), _nan(n * V + 64)
        lsm[n * V:], comb[n * V:] = SENTINEL, SENTINEL
        lib.call('re2e_lm_log_softmax_combine', x.data_ptr(), n, V, att.data_ptr() if with_att else None, w, lsm.data_ptr(), comb.data_ptr() if with_att else None)
        torch.cuda.synchronize()
        assert bool((lsm[n * V:] == SENTINEL).all()) and bool((comb[n * V:] == SENTINEL).all())
        got = lsm[:n * V].view(n, V).cpu()
        assert bool(torch.isfinite(got).all())
        _held('V%d-n%d%s' % (V, n, '-att' if with_att else ''), 'lsm', got, l64, l32, R.BAR_GRAD)
        if with_att:
            assert torch.equal(got, alone), 'the log-probabilities must not depend on whether the combined score is asked for'
            want = R.comb_fp32(d['att'], w, got)
            assert torch.equal(comb[:n * V].view(n, V).cpu(), want), 'comb is not att + fl(w * lsm), two roundings'
        else:
            assert bool(torch.isnan(comb[:n * V]).all())
            alone = got
    for a, c in ((att.data_ptr(), None), (None, comb.data_ptr())):
        with pytest.raises(lib.Re2eError):
            lib.call('re2e_lm_log_softmax_combine', x.data_ptr(), n, V, a, w, lsm.data_ptr(), c)


@pytest.mark.parametrize('n,ncand', [(1, 1), (5, 51), (4, 64), (1, 257), (64, 64)])
def test_lm_add_cands_bitwise(n, ncand):
    """local += w * lm[row][cand], bitwise the fp32 gather-multiply-add (two roundings); labels -1 and V give NaN there and nowhere else; what
    lies behind the n * ncand entries is not touched: a band of a finite sentinel (a NaN would swallow a stray += unseen), then a band of NaN,
    both with valid labels under them."""
    ops, lib = _ops()
    V, w, band = 37, 0.3, 300
    g = torch.Generator().manual_seed(100 * n + ncand)
    total = n * ncand
    lm = torch.log_softmax(R.rnd(g, n + band // ncand + 2, V), 1)
    cand = torch.randint(0, V, (total + band,), generator=g).to(torch.int32)
    local = R.rnd(g, total + band)
    local[total:total + band // 2] = SENTINEL
    local[total + band // 2:] = NAN
    for with_bad in (False, True):
        cd = cand.clone()
        if with_bad:
            cd[0] = -1
            cd[total - 1] = V
            if total > 2:
                cd[total // 2] = V + 5
        want = R.add_cands_fp32(local[:total].view(n, ncand), lm[:n], cd[:total].view(n, ncand), w)
        loc_d, lm_d, cd_d = local.to(DEV), lm.to(DEV), cd.to(DEV)
        lib.call('re2e_lm_add_cands', loc_d.data_ptr(), lm_d.data_ptr(), cd_d.data_ptr(), n, ncand, V, w)
        got = loc_d.cpu()
        assert int(torch.isnan(want).sum()) == (0 if not with_bad else len({0, total - 1, total // 2} if total > 2 else {0, total - 1}))
        assert torch.equal(torch.isnan(got[:total]), torch.isnan(want.view(-1)))
        ok = ~torch.isnan(want.view(-1))
        assert torch.equal(got[:total][ok], want.view(-1)[ok]), (got[:total][ok] - want.view(-1)[ok]).abs().max()
        assert bool((got[total:total + band // 2] == SENTINEL).all()) and bool(torch.isnan(got[total + band // 2:]).all()), 'entries behind n * ncand were touched'
