"""Beam search over several utterances at once (E2E.recognize_batch, model/beam_search.py recognize_beam_batch) and its three kernels:
re2e_attloc_fwd_rows and re2e_ctc_prefix_score_batch against their single-utterance siblings, bit for bit; re2e_beam_prune against a
numpy restatement of recognize_beam's host pruning loop (itself checked on the CPU against a literal copy of that loop); the n-best lists
against the reference's own (tests/golden/recog_tiny.npz, recog_lm_tiny.npz) and against ``recognize`` utterance by utterance."""
import argparse

import numpy as np
import pytest
import torch

from test_modules_gpu import DEV, _fx, _load, _opt

gpu = pytest.mark.gpu
CHARS = [str(i) for i in range(12)]
V_FULL = 4233


def _args(beam, penalty, ctcw, maxr, minr, nbest, lm_weight=0.0):
    return argparse.Namespace(beam_size=beam, penalty=penalty, ctc_weight=ctcw, maxlenratio=maxr, minlenratio=minr, nbest=nbest, lm_weight=lm_weight)


# ---- the pruning order -----------------------------------------------------------------------------------------------------------
def host_loop(hyp, local, beam):
    """A literal copy of recognize_beam's ``kept`` loop for the rows of ONE utterance: [(parent, column, score)]."""
    from robust_e2e_gan_amd.model.beam_search import _topk
    kept = []
    for k in range(len(hyp)):
        best_scores, joint = _topk(local[k], beam)
        for j in range(len(joint)):
            kept.append({'score': np.float32(hyp[k] + best_scores[j]), 'parent': k, 'col': int(joint[j])})
        kept = sorted(kept, key=lambda x: x['score'], reverse=True)[:beam]
    return [(h['parent'], h['col'], h['score']) for h in kept]


def prune_restated(hyp, local, beam):
    """The same list as one sort: score descending, then parent row ascending, then local descending, then column ascending."""
    rows, ncand = local.shape
    s = (hyp[:, None] + local).astype(np.float32)                       # one fp32 addition per entry
    r, c = np.divmod(np.arange(rows * ncand), ncand)
    order = np.lexsort((c, -local.reshape(-1), r, -s.reshape(-1)))[:beam]       # (the last key is the primary one)
    return [(int(r[o]), int(c[o]), s.reshape(-1)[o]) for o in order]


def _prune_inputs(rng, rows, ncand, kind):
    if kind == 'quarter':                       # multiples of 0.25: ties across rows and columns are frequent
        hyp = (rng.integers(-12, 1, rows) * 0.25).astype(np.float32)
        local = (rng.integers(-16, 1, (rows, ncand)) * 0.25).astype(np.float32)
    else:                                       # 'collapse': |hyp| ~ 1024 (ulp 2^-13 ... 2^-12), locals multiples of 2^-20 -> distinct locals, equal sums
        hyp = (-1024.0 - rng.integers(0, 3, rows) * 2.0 ** -13).astype(np.float32)
        local = (-rng.integers(0, 1 << 14, (rows, ncand)) * 2.0 ** -20).astype(np.float32)
    return hyp, local


def test_prune_restatement_is_the_host_loop():
    """CPU: the four-key order against the literal host loop on ragged cases with heavy ties, including sums that collapse under fp32
    rounding (where the third key decides)."""
    rng = np.random.default_rng(7)
    collapsed = 0
    for case in range(600):
        beam = int(rng.integers(1, 13))
        rows = int(rng.integers(1, beam + 1))
        ncand = int(rng.integers(1, 30))
        kind = 'quarter' if case % 3 else 'collapse'
        hyp, local = _prune_inputs(rng, rows, ncand, kind)
        want, got = host_loop(hyp, local, beam), prune_restated(hyp, local, beam)
        assert len(got) == len(want) == min(beam, rows * ncand)
        for a, b in zip(got, want):
            assert a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes(), (case, kind, got, want)
        if kind == 'collapse':
            collapsed += any(x[2] == y[2] and x[0] == y[0] and local[x[0], x[1]] != local[y[0], y[1]] for x, y in zip(got, got[1:]))
    assert collapsed > 20, 'the collapse cases never produced equal sums from different locals of one hypothesis'


@gpu
@pytest.mark.parametrize('kind', ['quarter', 'collapse'])
@pytest.mark.parametrize('ncand', [18, V_FULL])
@pytest.mark.parametrize('beam', [1, 3, 12])
def test_beam_prune_matches_host_loop_order(beam, ncand, kind):
    """re2e_beam_prune on segments of (1, beam, beam - 1) rows: parents, columns and labels exact, scores bitwise, counts, and the defined
    tail (-1 / -inf) where an utterance has fewer than ``beam`` continuations; outputs start as NaN / a sentinel.  ncand = 18 with a label
    list, ncand = V = 4233 with the column as the label."""
    from robust_e2e_gan_amd.lib import call
    rng = np.random.default_rng(100 * beam + ncand % 97 + (kind == 'collapse'))
    segs = [1, beam, beam - 1]
    seg = np.concatenate([[0], np.cumsum(segs)]).astype(np.int32)
    nh, U = int(seg[-1]), 3
    hyp, local = _prune_inputs(rng, nh, ncand, kind)
    cand = rng.integers(0, V_FULL, (nh, ncand)).astype(np.int32) if ncand != V_FULL else None
    d = lambda a: torch.from_numpy(a).to(DEV)
    seg_d, hyp_d, local_d, cand_d = d(seg), d(hyp), d(local), (d(cand) if cand is not None else None)
    ints = torch.full((3, U, beam), -777, dtype=torch.int32, device=DEV)
    score = torch.full((U, beam), float('nan'), device=DEV)
    count = torch.full((U,), -777, dtype=torch.int32, device=DEV)
    kk = min(beam, ncand)
    ws = torch.empty(2 * nh * kk, dtype=torch.int32, device=DEV)
    call('re2e_beam_prune', seg_d.data_ptr(), U, max(segs), hyp_d.data_ptr(), local_d.data_ptr(), cand_d.data_ptr() if cand_d is not None else None, nh,
         ncand, beam, ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), score.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel() * 4)
    ints, score, count = ints.cpu().numpy(), score.cpu().numpy(), count.cpu().numpy()
    for u in range(U):
        r0, r1 = int(seg[u]), int(seg[u + 1])
        want = prune_restated(hyp[r0:r1], local[r0:r1], beam) if r1 > r0 else []
        assert count[u] == len(want) == min(beam, (r1 - r0) * ncand), (u, count[u], len(want))
        for k, (par, col, s) in enumerate(want):
            lab = int(cand[r0 + par, col]) if cand is not None else col
            assert (ints[0, u, k], ints[1, u, k], ints[2, u, k]) == (r0 + par, col, lab), (u, k, ints[:, u, k], (r0 + par, col, lab))
            assert score[u, k].tobytes() == s.tobytes(), (u, k, score[u, k], s)
        assert (ints[:, u, len(want):] == -1).all() and (score[u, len(want):] == -np.inf).all(), (u, ints[:, u], score[u])


@gpu
def test_beam_prune_limits():
    from robust_e2e_gan_amd.lib import call_supported
    z = torch.zeros(70 * 70, device=DEV)
    zi = torch.zeros(70 * 70, dtype=torch.int32, device=DEV)
    a = lambda nrows, beam: call_supported('re2e_beam_prune', zi.data_ptr(), 1, nrows, z.data_ptr(), z.data_ptr(), None, nrows, 4, beam, zi.data_ptr(),
                                           zi.data_ptr(), zi.data_ptr(), z.data_ptr(), zi.data_ptr(), z.data_ptr(), z.numel() * 4)
    assert a(3, 65) is False               # beam > 64
    assert a(5, 4) is False                # more rows than `beam` in an utterance


# ---- the prefix scorer ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('out_len', [0, 1, 3])
@pytest.mark.parametrize('V,ctc_beam', [(12, 6), (V_FULL, 15)])
def test_ctc_prefix_score_batch_matches_single(V, ctc_beam, out_len):
    """Tmax = 37, T_u = (37, 29, 3), rows of utterances (2, 0, 0, 1, 2): candidates exact, local and prefix scores and r_new[:, :, :T_u]
    bitwise those of re2e_ctc_prefix_score on each utterance alone (its own T, contiguous operands); r_new at t >= T_u written (-1e10).
    Row 1 has its last label among its candidates (the repeat branch), row 0 -- of the 3-frame utterance -- and row 3 have <eos> among
    theirs (rsum[T_u - 1]: where a Tmax would slip in).  Outputs start as NaN; r_prev beyond T_u holds a finite decoy."""
    from robust_e2e_gan_amd.lib import call
    g = torch.Generator().manual_seed(1000 + V + out_len)
    Tmax, Ts, utt = 37, [37, 29, 3], [2, 0, 0, 1, 2]
    U, nh, eos = 3, 5, V - 1
    lpz = torch.log_softmax(torch.randn(U, Tmax, V, generator=g), 2)
    for u in range(U):
        lpz[u, Ts[u]:] = 0.0
    att = torch.log_softmax(torch.randn(nh, V, generator=g), 1)
    last = torch.randint(1, V - 1, (nh,), generator=g, dtype=torch.int32)
    att[1, int(last[1])] = 0.5                              # the repeat branch (taken when out_len > 0)
    att[0, eos] = att[3, eos] = 0.25
    r_prev = torch.full((nh, Tmax, 2), 123.0)
    for h, u in enumerate(utt):
        if out_len == 0:
            r_prev[h, :Ts[u], 0] = -1e10
            r_prev[h, :Ts[u], 1] = torch.cumsum(lpz[u, :Ts[u], 0], 0)
        else:
            r_prev[h, :Ts[u]] = -10.0 * torch.rand(Ts[u], 2, generator=g) - 0.1
    olen = torch.full((nh,), out_len, dtype=torch.int32)
    prev = -torch.rand(nh, generator=g) * (1.0 if out_len else 0.0)
    aw, cw = float(np.float32(0.7)), float(np.float32(0.3))
    D = lambda t: t.contiguous().to(DEV)
    lpz_d, att_d, last_d, olen_d, prev_d, r_prev_d = D(lpz), D(att), D(last), D(olen), D(prev), D(r_prev)
    nan = lambda *s: torch.full(s, float('nan'), device=DEV)
    cand = torch.full((nh, ctc_beam), -777, dtype=torch.int32, device=DEV)
    loc, pfx, r_new = nan(nh, ctc_beam), nan(nh, ctc_beam), nan(nh, ctc_beam, Tmax, 2)
    tl_d, utt_d = D(torch.tensor(Ts, dtype=torch.int32)), D(torch.tensor(utt, dtype=torch.int32))
    call('re2e_ctc_prefix_score_batch', lpz_d.data_ptr(), U, Tmax, V, tl_d.data_ptr(), utt_d.data_ptr(), att_d.data_ptr(), nh, r_prev_d.data_ptr(), last_d.data_ptr(), olen_d.data_ptr(), prev_d.data_ptr(),
         ctc_beam, aw, cw, 0, eos, cand.data_ptr(), loc.data_ptr(), pfx.data_ptr(), r_new.data_ptr())
    seen_rep = seen_eos = False
    for u in range(U):
        rows = [h for h in range(nh) if utt[h] == u]
        n, T = len(rows), Ts[u]
        idx = torch.tensor(rows, device=DEV)
        c1 = torch.full((n, ctc_beam), -777, dtype=torch.int32, device=DEV)
        l1, p1, rn1 = nan(n, ctc_beam), nan(n, ctc_beam), nan(n, ctc_beam, T, 2)
        ops1 = [lpz_d[u, :T].contiguous(), att_d[idx].contiguous(), r_prev_d[idx][:, :T].contiguous(), last_d[idx].contiguous(), olen_d[idx].contiguous(),
                prev_d[idx].contiguous()]                    # (held: a temporary's memory would be handed to the next one)
        call('re2e_ctc_prefix_score', ops1[0].data_ptr(), T, V, ops1[1].data_ptr(), n, ops1[2].data_ptr(), ops1[3].data_ptr(), ops1[4].data_ptr(),
             ops1[5].data_ptr(), ctc_beam, aw, cw, 0, eos, c1.data_ptr(), l1.data_ptr(), p1.data_ptr(), rn1.data_ptr())
        assert torch.equal(cand[idx], c1), (u, cand[idx], c1)
        assert torch.equal(loc[idx], l1) and torch.equal(pfx[idx], p1), (u, (loc[idx] - l1).abs().max(), (pfx[idx] - p1).abs().max())
        assert bool(torch.isfinite(l1).all()) and bool(torch.isfinite(p1).all())
        assert torch.equal(r_new[idx][:, :, :T], rn1), (u, 'r_new over t < T_u')
        assert bool((r_new[idx][:, :, T:] == -1e10).all()), (u, 'r_new at t >= T_u is not written')
        for k, h in enumerate(rows):
            seen_rep |= out_len > 0 and int(last[h]) in c1[k].tolist()
            seen_eos |= eos in c1[k].tolist()
    assert seen_eos and (seen_rep or out_len == 0)


# ---- the attention step -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('with_prev', [False, True])
@pytest.mark.parametrize('E,Dn,A,C,Fh', [(20, 14, 18, 4, 5), (320, 300, 320, 10, 100)])
def test_attloc_fwd_rows_matches_single(E, Dn, A, C, Fh, with_prev):
    """T = 37 (a full 32-frame chunk and a partial one), lengths (37, 29, 20), rows of utterances (2, 0, 0, 1, 2), pre / enc held once per
    utterance: w, c, conv_out over each row's own frames and dp_out are bitwise what re2e_attloc_fwd gives for that utterance alone on
    inputs replicated per row, as the single-utterance search replicates them (T = T_u: a row of a shorter utterance has only its own
    frames; re2e_attloc_fwd itself, with T = 37, would spread the softmax over the padding).  Weights and conv_out beyond each length are
    zero.  Outputs start as NaN; a given att_prev holds a decoy beyond each length."""
    from robust_e2e_gan_amd.lib import call
    g = torch.Generator().manual_seed(50 + E + int(with_prev))
    T, Ts, utt = 37, [37, 29, 20], [2, 0, 0, 1, 2]
    U, nh = 3, 5
    R = lambda *s: torch.randn(*s, generator=g)
    pre, enc = R(U, T, A), R(U, T, E)
    for u in range(U):
        pre[u, Ts[u]:], enc[u, Ts[u]:] = 0.0, 0.0
    z = R(nh, Dn)
    att_prev = None
    if with_prev:
        att_prev = torch.full((nh, T), 0.5)
        for h, u in enumerate(utt):
            att_prev[h, :Ts[u]] = torch.softmax(R(Ts[u]), 0)
    w_decT, w_att, w_conv, gvec, gb = R(Dn, A) * 0.2, R(A, C) * 0.3, R(C, 2 * Fh + 1) * 0.3, R(A) * 0.3, R(1)
    D = lambda t: t.contiguous().to(DEV)
    pre_d, enc_d, z_d, ap_d = D(pre), D(enc), D(z), (D(att_prev) if with_prev else None)
    wd, wa, wc, gv, gbd = D(w_decT), D(w_att), D(w_conv), D(gvec), D(gb)
    nan = lambda *s: torch.full(s, float('nan'), device=DEV)
    w, cx, conv, dp, es = nan(nh, T), nan(nh, E), nan(nh, T, C), nan(nh, A), nan(nh, T)
    tl_d, utt_d = D(torch.tensor(Ts, dtype=torch.int32)), D(torch.tensor(utt, dtype=torch.int32))
    call('re2e_attloc_fwd_rows', pre_d.data_ptr(), enc_d.data_ptr(), U, tl_d.data_ptr(), utt_d.data_ptr(), z_d.data_ptr(), ap_d.data_ptr() if with_prev else None, wd.data_ptr(), wa.data_ptr(),
         wc.data_ptr(), gv.data_ptr(), gbd.data_ptr(), nh, T, E, Dn, A, C, Fh, w.data_ptr(), cx.data_ptr(), E, conv.data_ptr(), dp.data_ptr(), es.data_ptr())
    for u in range(U):
        rows = [h for h in range(nh) if utt[h] == u]
        n, Tu = len(rows), Ts[u]
        idx = torch.tensor(rows, device=DEV)
        pre_r, enc_r = pre_d[u, :Tu].unsqueeze(0).expand(n, Tu, A).contiguous(), enc_d[u, :Tu].unsqueeze(0).expand(n, Tu, E).contiguous()
        ap_r = ap_d[idx][:, :Tu].contiguous() if with_prev else None
        z_r = z_d[idx].contiguous()
        w1, c1, cv1, dp1, es1 = nan(n, Tu), nan(n, E), nan(n, Tu, C), nan(n, A), nan(n, Tu)
        hl_r = D(torch.tensor([Tu] * n, dtype=torch.int32))
        call('re2e_attloc_fwd', pre_r.data_ptr(), enc_r.data_ptr(), z_r.data_ptr(), ap_r.data_ptr() if with_prev else None, hl_r.data_ptr(), wd.data_ptr(), wa.data_ptr(), wc.data_ptr(), gv.data_ptr(), gbd.data_ptr(), n, Tu, E,
             Dn, A, C, Fh, w1.data_ptr(), c1.data_ptr(), E, cv1.data_ptr(), dp1.data_ptr(), es1.data_ptr())
        assert bool(torch.isfinite(w1).all()) and bool(torch.isfinite(c1).all())
        assert torch.equal(dp[idx], dp1), (u, 'dp_out')
        assert torch.equal(conv[idx][:, :Tu], cv1), (u, 'conv_out', (conv[idx][:, :Tu] - cv1).abs().max())
        assert torch.equal(w[idx][:, :Tu], w1), (u, 'w', (w[idx][:, :Tu] - w1).abs().max())
        assert torch.equal(cx[idx], c1), (u, 'c', (cx[idx] - c1).abs().max())
        assert bool((w[idx][:, Tu:] == 0).all()) and bool((conv[idx][:, Tu:] == 0).all()), (u, 'beyond the length')


# ---- the search -------------------------------------------------------------------------------------------------------------------
def _tiny(golden_dir):
    from robust_e2e_gan_amd.model.e2e_model import E2E
    base = _fx(golden_dir, 'recog_tiny.npz')
    return base, _load(E2E(_opt()), base, 'p.'), torch.from_numpy(base['feats']), base['lens'].tolist()


@gpu
def test_recognize_batch_matches_reference_nbest(golden_dir):
    """The three utterances of recog_tiny.npz (37 / 29 / 20 frames) as ONE padded batch reproduce the reference's n-best lists for the
    four search configurations (joint_ratio: per-utterance maxlen / minlen)."""
    from test_oracle_golden import RECOG_CONFIGS, check_nbest
    base, asr, feats, lens = _tiny(golden_dir)
    assert lens == [37, 29, 20]
    for name, beam, penalty, ctcw, maxr, minr, nbest in RECOG_CONFIGS:
        got = asr.recognize_batch(feats, lens, _args(beam, penalty, ctcw, maxr, minr, nbest), CHARS)
        assert len(got) == 3
        for u in range(3):
            check_nbest(got[u], base, name, u)
    assert asr.training                                                  # mode restored


@gpu
def test_recognize_batch_with_lm_matches_reference_nbest(golden_dir):
    """... and with the reference's RNNLM (recog_lm_tiny.npz): the configurations and lm_weight values of test_recog_lm_gpu.py --
    attention-only + LM, joint + LM, and ctc_weight = 1.0, which takes the per-utterance fallback."""
    from test_oracle_golden import RECOG_CONFIGS, check_nbest
    from test_recog_lm_gpu import LM_CONFIGS_EXTRA, LM_WEIGHTS, _tiny_lm
    base, asr, feats, lens = _tiny(golden_dir)
    fx = _fx(golden_dir, 'recog_lm_tiny.npz')
    lm = _tiny_lm(fx)
    for name, beam, penalty, ctcw, maxr, minr, nbest in RECOG_CONFIGS + LM_CONFIGS_EXTRA:
        for w in LM_WEIGHTS:
            got = asr.recognize_batch(feats, lens, _args(beam, penalty, ctcw, maxr, minr, nbest, w), CHARS, rnnlm=lm)
            for u in range(3):
                check_nbest(got[u], fx, '%s.w%03d' % (name, int(round(w * 100))), u)


def _same(a, b, tol):
    assert len(a) == len(b), (len(a), len(b))
    for x, y in zip(a, b):
        assert x['yseq'] == y['yseq'], (x['yseq'], y['yseq'])
        assert abs(x['score'] - y['score']) <= tol * max(1.0, abs(y['score'])), (x['score'], y['score'])


@gpu
@pytest.mark.parametrize('name', ['joint_b4', 'att_b3'])
def test_recognize_batch_utterances_are_independent(golden_dir, name):
    """A segment offset or a T'max that leaks between utterances shows here: the batch in the order (2, 0, 1) returns the permuted lists;
    U = 1 is ``recognize`` (the same launches on the same rows: equal scores); in the batch (u0, u0, u2) the two copies of u0 return
    identical lists and u2 its own.  Between batches of different composition the products see other row counts and may run on another
    plan, so scores are compared to 1e-5 (fp32 sums of a few log-probabilities of magnitude <= 10: 100 ulp), the label sequences exactly."""
    from test_oracle_golden import RECOG_CONFIGS
    base, asr, feats, lens = _tiny(golden_dir)
    asr.eval()
    cfg = [c for c in RECOG_CONFIGS if c[0] == name][0]
    args = _args(*cfg[1:])
    inorder = asr.recognize_batch(feats, lens, args, CHARS)
    assert not asr.training                                              # mode restored
    perm = [2, 0, 1]
    got = asr.recognize_batch(feats[perm], [lens[u] for u in perm], args, CHARS)
    for j, u in enumerate(perm):
        _same(got[j], inorder[u], 1e-5)
    for u in range(3):
        one = asr.recognize_batch(feats[u:u + 1, :lens[u]], [lens[u]], args, CHARS)
        _same(one[0], asr.recognize(feats[u:u + 1, :lens[u]], args, CHARS), 0.0)
        _same(one[0], inorder[u], 1e-5)
    dup = asr.recognize_batch(feats[[0, 0, 2]], [lens[0], lens[0], lens[2]], args, CHARS)
    _same(dup[0], dup[1], 0.0)
    _same(dup[0], inorder[0], 1e-5)
    _same(dup[2], inorder[2], 1e-5)


FULL_SEEDS = (21, 4)          # model, utterances: those of test_recognize_full_width_device_ctc_vs_host_ctc


@gpu
@pytest.mark.parametrize('ctc_weight', [0.3, 0.0])
def test_recognize_batch_full_width(ctc_weight):
    """The config-4 width (V = 4233) on three random utterances of 800 / 640 / 400 frames (T' = 200 / 160 / 100), beam 10: joint search
    (ctc_weight 0.3, maxlenratio 0.08) and attention-only search with the recipe's LM (256 / 650 units, lm_weight 0.2, maxlenratio 0.03)
    return, utterance by utterance, ``recognize``'s label sequences with scores within 2e-3 * max(1, |score|) (the batched products see
    more rows and may take another plan).  Seeds: model 21, utterances 4 (those of test_recognize_full_width_device_ctc_vs_host_ctc), LM 22.
    Adjacent n-best scores of ``recognize`` alone are CLOSER than that tolerance here, and no seed changes that: with utterance seeds
    1 .. 24 the smallest adjacent gap was 0.00 - 0.20 of the tolerance for the joint search (scores near -125.5) and 0.00 - 0.09 for the
    LM search (near -56.2) -- a freshly initialised model ranks its hypotheses almost flat -- so the order compared is decided by less
    than the score tolerance on every seed.  It is decided all the same: on all 24 seeds and both configurations the batched search
    returned ``recognize``'s sequences with score differences of exactly 0.  The gaps are printed, not asserted."""
    from robust_e2e_gan_amd.joint_train import config4_opt
    from robust_e2e_gan_amd.model.e2e_model import E2E
    from robust_e2e_gan_amd.model.lm import RNNLM, ClassifierWithState
    opt = config4_opt()
    torch.manual_seed(FULL_SEEDS[0])
    asr = E2E(opt).to(DEV)
    lm = None
    if ctc_weight == 0.0:
        torch.manual_seed(22)
        lm = ClassifierWithState(RNNLM(opt.odim, 256, 650))
        lm.predictor.lo.weight.data.uniform_(-0.5, 0.5)
        lm = lm.to(DEV).eval()
    g = torch.Generator().manual_seed(FULL_SEEDS[1])
    lens = [800, 640, 400]
    feats = torch.randn(3, 800, 80, generator=g)
    for u in range(3):
        feats[u, lens[u]:] = 0.0
    args = _args(10, 0.0, ctc_weight, 0.08 if ctc_weight else 0.03, 0.0, 5, 0.2)
    single = [asr.recognize(feats[u:u + 1, :lens[u]], args, opt.char_list, rnnlm=lm) for u in range(3)]
    for u, nb in enumerate(single):
        assert len(nb) == 5
        for a, b in zip(nb, nb[1:]):
            gap, tol = a['score'] - b['score'], 2e-3 * max(1.0, abs(b['score']))
            print('ctc_weight %.1f utterance %d: adjacent n-best gap %.4g (tolerance %.4g)' % (ctc_weight, u, gap, tol))
    got = asr.recognize_batch(feats, lens, args, opt.char_list, rnnlm=lm)
    for u in range(3):
        _same(got[u], single[u], 2e-3)
