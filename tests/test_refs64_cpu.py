"""Pins the float64 references of tests/refs64.py (CPU only): the written-out decoder loop against attention weights that came from the
reference's own modules, the cross-entropy / label-smoothing references against the oracle's decoder loss, and -- for every input of
tests/test_loss_kernels_gpu.py -- that torch's own fp32 run of the same reference stays within a quarter of the bar the HIP kernels are
held to there (a bar that fp32 arithmetic cannot meet on its input would say nothing about a kernel)."""
import os

import numpy as np
import pytest
import torch

import refs64 as R


def _fx(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name), allow_pickle=False))


def _loop_inputs(p, hpad, hlens, ys, eos, dtype):
    """What model/e2e_decoder.py hands to the loop: masked encoder states, their projection, the tokens fed (sos first), and the targets."""
    B, T, _ = hpad.shape
    L1 = max(len(y) for y in ys) + 1
    ids_in = torch.full((B, L1), eos, dtype=torch.long)
    ids_out = torch.full((B, L1), -1, dtype=torch.long)
    for b, y in enumerate(ys):
        ids_in[b, 1:len(y) + 1] = y
        ids_out[b, :len(y)] = y
        ids_out[b, len(y)] = eos
    d = lambda k: p[k].detach().to(dtype)
    hmask = hpad.detach().to(dtype) * (torch.arange(T).unsqueeze(0) < torch.tensor(hlens).unsqueeze(1)).unsqueeze(2).to(dtype)
    pre = hmask @ d('att.mlp_enc.weight').t() + d('att.mlp_enc.bias')
    Pm = dict(embed=d('dec.embed.weight'), w_ih=d('dec.decoder.0.weight_ih'), w_hh=d('dec.decoder.0.weight_hh'), b_ih=d('dec.decoder.0.bias_ih'),
              b_hh=d('dec.decoder.0.bias_hh'), mlp_dec=d('att.mlp_dec.weight'), mlp_att=d('att.mlp_att.weight'), loc_conv=d('att.loc_conv.weight'),
              gvec_w=d('att.gvec.weight'), gvec_b=d('att.gvec.bias'))
    return hmask, pre, ids_in.t().contiguous(), ids_out.t().contiguous(), L1, Pm


def _close(name, got, ref, tol):
    err = (got.double() - ref.double()).abs().max().item()
    scale = ref.double().abs().max().item()
    assert err <= tol * scale + 1e-6, '%s: max err %.3e vs scale %.3e' % (name, err, scale)


@pytest.mark.parametrize('tag', ['a.', 'b.'])
def test_decoder_loop_ref_reproduces_reference_attention_weights(golden_dir, tag):
    """dec_persist_tiny.npz holds att_w of every step from a forward hook on the reference's AttLoc (make_fixtures_dec.py)."""
    fx = _fx(golden_dir, 'dec_persist_tiny.npz')
    p = {}
    for k, v in fx.items():
        if k.startswith(tag + 'p.dec.'):
            n = k[len(tag) + 2:]
            p[n[4:] if n.startswith('dec.att.') else n] = torch.from_numpy(v)
    tl, ys, o = fx[tag + 'tlens'].tolist(), [], 0
    for n in tl:
        ys.append(torch.from_numpy(fx[tag + 'ys'][o:o + n]))
        o += n
    hlens = fx[tag + 'hlens'].tolist()
    hmask, pre, ids, tgt, L1, Pm = _loop_inputs(p, torch.from_numpy(fx[tag + 'hpad']), hlens, ys, 11, torch.float64)
    zs, w = R.decoder_loop_ref(hmask, pre, ids, hlens, L1, Pm)
    _close('att_w', w.transpose(0, 1), torch.from_numpy(fx[tag + 'att_w']), 1e-4)
    # and the loss the reference recorded, through the cross-entropy reference
    logits = zs.reshape(L1 * len(hlens), -1) @ p['dec.output.weight'].double().t() + p['dec.output.bias'].double()
    loss, _, _, _ = R.ce_ref(logits, tgt.reshape(-1), float(np.mean([n + 1 for n in tl])) - 1.0)
    _close('loss_att', loss.view(1), torch.from_numpy(fx[tag + 'loss_att']), 1e-4)


def test_refs_reproduce_oracle_decoder_on_e2e_tiny(golden_dir):
    """e2e_tiny.npz: attention weights, loss (with and without label smoothing) and accuracy of oracle.nets.decoder_forward, which
    test_oracle_golden.py pins to the reference's recorded loss_att."""
    from oracle import nets
    fx = _fx(golden_dir, 'e2e_tiny.npz')
    p = {k[2:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith('p.') and not k.startswith('p.dec.att.')}
    hpad, hlens = torch.from_numpy(fx['hpad']), fx['hlens'].tolist()
    tl = fx['tlens'].tolist()
    ys = nets.split_targets(torch.from_numpy(fx['targets']), tl)
    V = p['dec.output.weight'].shape[0]
    g = torch.Generator().manual_seed(3)
    labeldist = torch.rand(V, generator=g) / V
    labeldist[2] = 0.0
    loss_o, acc_o, att_o = nets.decoder_forward(p, hpad, hlens, ys, V - 1, return_att=True)
    loss_l, _ = nets.decoder_forward(p, hpad, hlens, ys, V - 1, labeldist=labeldist, lsm_weight=0.3)
    hmask, pre, ids, tgt, L1, Pm = _loop_inputs(p, hpad, hlens, ys, V - 1, torch.float64)
    zs, w = R.decoder_loop_ref(hmask, pre, ids, hlens, L1, Pm)
    _close('att_w', w.transpose(0, 1), att_o, 1e-4)
    B = len(hlens)
    logits = zs.transpose(0, 1).reshape(B * L1, -1) @ p['dec.output.weight'].double().t() + p['dec.output.bias'].double()       # the oracle's rows are batch-major
    tgt_bm = tgt.t().reshape(-1)
    loss, correct, valid, _ = R.ce_ref(logits, tgt_bm, float(np.mean([n + 1 for n in tl])) - 1.0)
    _close('loss', loss.view(1), loss_o.detach().view(1), 1e-4)
    _close('loss vs recorded', loss.view(1), torch.from_numpy(fx['loss_att']).view(1), 1e-4)
    assert abs(correct / valid - acc_o) < 1e-9 and valid == sum(tl) + B
    reg, _ = R.lsm_ref(logits, labeldist, B)
    _close('loss with label smoothing', (0.7 * loss + 0.3 * reg).view(1), loss_l.detach().view(1), 1e-4)


def test_argmax_tie_goes_to_the_lower_index():
    x = torch.tensor([[1.0, 5.0, 5.0, 0.0], [7.0, 2.0, 7.0, 7.0], [0.0, 0.0, 0.0, 3.0]], dtype=torch.float64)
    assert R.argmax_first(x).tolist() == [1, 0, 3]
    loss, correct, valid, _ = R.ce_ref(x, torch.tensor([2, 0, -1]), 1.0)
    assert (correct, valid) == (1, 2)


def test_embedding_bwd_ref_sums_duplicates_and_accumulates():
    dout = torch.tensor([[1.0, 2.0], [10.0, 20.0], [100.0, 200.0]])
    got = R.embedding_bwd_ref(dout, torch.tensor([2, 0, 2]), 4, beta=1.0, prev=torch.ones(4, 2))
    assert got.tolist() == [[11.0, 21.0], [1.0, 1.0], [102.0, 203.0], [1.0, 1.0]]


def test_ctc_ref_infeasible_alignment_is_inf_with_nan_rows():
    c = R.ctc_infeasible_case()
    for dtype in (torch.float64, torch.float32):
        nll, loss, d = R.ctc_ref(c['logits'], c['hlens'], c['labels'], dtype)
        assert not torch.isfinite(loss)
        for b in range(c['B']):
            h = c['hlens'][b]
            if b in c['infeasible']:
                assert nll[b] == float('inf') and torch.isnan(d[:h, b]).all()
            else:
                assert torch.isfinite(nll[b]) and torch.isfinite(d[:h, b]).all() and d[:h, b].abs().max() > 0
            assert (d[h:, b] == 0).all()


# ---------------------------------------------------------------------------------------------
# every bar of test_loss_kernels_gpu.py means something on its input: fp32 on the CPU meets it four times over
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(R.ctc_cases()))
def test_fp32_margin_ctc(name):
    c = R.ctc_cases()[name]
    n64, l64, d64 = R.ctc_ref(c['logits'], c['hlens'], c['labels'])
    n32, l32, d32 = R.ctc_ref(c['logits'], c['hlens'], c['labels'], torch.float32)
    R.margin_ok('loss', l32, l64, R.BAR_LOSS)
    R.margin_ok('nll', n32, n64, R.BAR_LOSS)
    R.margin_ok('dlogits', d32, d64, R.BAR_GRAD)


@pytest.mark.parametrize('R_,V', R.SEQLOSS_SHAPES)
def test_fp32_margin_seqloss(R_, V):
    c = R.seqloss_case(R_, V)
    l64, k64, v64, d64 = R.ce_ref(c['x'], c['targets'], c['scale'])
    l32, k32, v32, d32 = R.ce_ref(c['x'], c['targets'], c['scale'], torch.float32)
    assert (k32, v32) == (k64, v64) and 0 < v64 < R_
    R.margin_ok('ce loss', l32, l64, R.BAR_LOSS)
    R.margin_ok('ce dlogits', d32, d64, R.BAR_GRAD)
    r64, e64 = R.lsm_ref(c['x'], c['dist'], c['nutt'])
    r32, e32 = R.lsm_ref(c['x'], c['dist'], c['nutt'], torch.float32)
    R.margin_ok('lsm', r32, r64, R.BAR_LOSS)
    R.margin_ok('lsm dlogits', e32, e64, R.BAR_GRAD)
    R.margin_ok('log_softmax', c['x'].log_softmax(1), c['x'].double().log_softmax(1), R.BAR_LOSS)
    assert R.argmax_first(c['x'].double())[[0, 2, 3]].tolist() == [1, 0, 0]    # the three tie rows: the lower index wins


@pytest.mark.parametrize('n,D', R.EMB_CASES)
def test_fp32_margin_embedding(n, D):
    c = R.embedding_case(n, D)
    ids = c['ids'].long()
    assert 7 not in ids.tolist() and 8 not in ids.tolist() and (n < 200 or int((ids == 3).sum()) > 64)
    for beta in (0.0, 1.0):
        a = R.embedding_bwd_ref(c['dout'][:, :D], c['ids'], c['V'], beta, c['prev'])
        b = R.embedding_bwd_ref(c['dout'][:, :D], c['ids'], c['V'], beta, c['prev'], torch.float32)
        R.margin_ok('dtable', b, a, R.BAR_GRAD)


@pytest.mark.parametrize('upstream', R.DEC_UPSTREAM)
@pytest.mark.parametrize('shape', [s for s, _, _ in R.DEC_SHAPES], ids=lambda s: 'x'.join(str(v) for v in s))
def test_fp32_margin_decoder(shape, upstream):
    c = R.decoder_case(shape)
    a, b = R.decoder_ref_run(c, upstream=upstream), R.decoder_ref_run(c, torch.float32, upstream)
    for k in ('zs', 'w'):
        R.margin_ok(k, b[k], a[k], R.BAR_DEC_OUT)
    for k in sorted(a):
        if k not in ('zs', 'w', 'gvec_b'):
            R.margin_ok(k, b[k], a[k], R.BAR_DEC_GRAD, R.ATOL_DEC_GRAD)
    assert a['gvec_b'].abs().max().item() < 1e-12          # a shift of the energies does not move a softmax: the true gradient is zero
