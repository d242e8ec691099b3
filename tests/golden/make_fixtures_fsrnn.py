#!/usr/bin/env python3
"""Golden vectors for the FS-RNN language model: the reference's own ClassifierWithState(FSRNNLM(12, 6, L, 10, 10, 0.9, 0.5)) (model/fsrnn.py,
model/lm.py:26-109) on the CPU, for L = 2 and L = 3 fast layers, parameters uniform(-1, 1), compute_accuracy = False.  Keys are prefixed L2. / L3.

  lm.*       the parameters
  win.*      one window of T = 4 steps x B = 3 rows from the zero state in EVALUATION mode with gradients enabled (zoneout is then the
             deterministic blend): per-step losses, the final state, the gradient of the summed loss for every parameter
  train.*    three iterations of the reference's loop body (lm.py:284-313) with dropout_rate = 0 and both keeps 1.0 -- its training mode
             is deterministic then -- on a 40-token corpus with batch 4 and bproplen 3: loss, gradient norm and parameters after each
             iteration.  GRADCLIP is chosen so that one step is clipped and one is not (asserted); an fp64 run must stay within 2.5e-4 of
             the fp32 one, a quarter of the 1e-3 parity bar (asserted).  train.valid_ppl: the reference's evaluation loop (lm.py:240-272)
             over a 16-token corpus with the window's model (keeps 0.9 / 0.5)
  chain.*    8 positions x 3 rows of ``predict`` with the permuted and repeated parents of make_fixtures_recog_lm.py
  <config>.<weight>.u<k>.yseq / .score   (L2 only) n-best lists of E2E.recognize(..., rnnlm=) on the model and utterances of
             recog_tiny.npz, over that file's search configurations at lm_weight 0.2 and 1.0; every list differs from its LM-free
             counterpart and adjacent scores are >= 1e-3 apart (asserted)

Runs only where the reference can be imported; writes fsrnn_tiny.npz.  No test imports this file."""
import argparse
import copy
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf   # noqa: E402
from make_fixtures_recog_lm import CHAIN_IDS, CHAIN_PARENTS, CONFIGS, LENS, LM_WEIGHTS, MIN_GAP, nbest_arrays, wtag   # noqa: E402

V, E, H = 12, 6, 10
KEEP_H, KEEP_C = 0.9, 0.5
WIN_T, WIN_B = 4, 3
CORPUS, VALID, BATCH, BPROPLEN, ITERS = 40, 16, 4, 3, 3
GRADCLIP = {2: 1.6, 3: 1.6}
QUARTER_BAR = 2.5e-4
STATE_KEYS = ('F_h', 'F_c', 'S_h', 'S_c')


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), 1e-30))


def zero_state(n, dtype):
    return {k: torch.zeros(n, H, dtype=dtype) for k in STATE_KEYS}


def loop_body(model, optimizer, it, state, clip):
    loss = 0
    for _ in range(BPROPLEN):
        batch = np.array(it.__next__())
        x, t = torch.from_numpy(batch[:, 0]).long(), torch.from_numpy(batch[:, 1]).long()
        state, loss_batch = model(state, x, t)
        loss += loss_batch
    model.zero_grad()
    loss.backward()
    for key in state.keys():
        state[key] = state[key].detach()
    norm = torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
    optimizer.step()
    return state, float(loss.detach()), float(norm)


def evaluate(model, it, dtype, bproplen=100):
    torch.set_grad_enabled(False)
    model.predictor.eval()
    state, sum_perp, data_count = zero_state(BATCH, dtype), 0, 0
    while True:
        try:
            batch = np.array(it.__next__())
        except StopIteration:
            break
        x, t = torch.from_numpy(batch[:, 0]).long(), torch.from_numpy(batch[:, 1]).long()
        state, loss = model(state, x, t)
        sum_perp += loss.data
        if data_count % bproplen == 0:
            for key in state.keys():
                state[key] = state[key].detach()
        data_count += 1
    torch.set_grad_enabled(True)
    model.predictor.train()
    return float(np.exp(float(sum_perp) / data_count))


def fresh_model(L, seed):
    from model.lm import ClassifierWithState
    from model.fsrnn import FSRNNLM
    torch.manual_seed(seed)
    lm = ClassifierWithState(FSRNNLM(V, E, L, H, H, KEEP_H, KEEP_C))
    lm.compute_accuracy = False
    for prm in lm.parameters():
        prm.data.uniform_(-1.0, 1.0)
    return lm


def one_model(L, seed, fx, report):
    from model.lm import ClassifierWithState
    from model.fsrnn import FSRNNLM
    from data.lm_data_loader import ParallelSequentialIterator
    pre = 'L%d.' % L
    lm = fresh_model(L, seed)
    fx.update(mf.sd_np(pre + 'lm.', lm))
    rng = np.random.RandomState(50 + L)

    # ---- one window, evaluation mode, gradients enabled -------------------------------------------------------------------------------
    lm.eval()
    xs, ts = rng.randint(0, V, (WIN_T, WIN_B)), rng.randint(0, V, (WIN_T, WIN_B))
    state, losses = None, []
    for t in range(WIN_T):
        state, loss = lm(state, torch.from_numpy(xs[t]).long(), torch.from_numpy(ts[t]).long())
        losses.append(loss)
    lm.zero_grad()
    sum(losses).backward()
    fx.update({pre + 'win.xs': xs.astype(np.int32), pre + 'win.ts': ts.astype(np.int32),
               pre + 'win.losses': np.array([float(v.detach()) for v in losses], np.float64)})
    fx.update({pre + 'win.state.' + k: v.detach().numpy().copy() for k, v in state.items()})
    fx.update(mf.grads_np(pre + 'win.grad.', lm))
    for k in range(2, L):
        g = lm.predictor.fast_cells[k].weight_ih.grad
        assert g is not None and float(g.abs().max()) == 0.0, 'fast_cells[%d].weight_ih.grad is expected to be a zero tensor' % k

    # ---- three training iterations with dropout 0 and keeps 1.0, in fp32 and in fp64 ---------------------------------------------------
    corpus, valid = rng.randint(0, V, CORPUS).astype(np.int32), rng.randint(0, V, VALID).astype(np.int32)
    fx.update({pre + 'train.corpus': corpus, pre + 'train.valid': valid, pre + 'train.gradclip': np.float64(GRADCLIP[L])})
    runs = {}
    for dtype in (torch.float32, torch.float64):
        m = ClassifierWithState(FSRNNLM(V, E, L, H, H, 1.0, 1.0, dropout_rate=0))
        m.compute_accuracy = False
        m.load_state_dict(copy.deepcopy(lm.state_dict()))
        m = m.to(dtype).train()
        opt = torch.optim.SGD(m.parameters(), lr=1.0)
        it = ParallelSequentialIterator(corpus, BATCH)
        state, rec = zero_state(BATCH, dtype), []
        for k in range(ITERS):
            state, loss, norm = loop_body(m, opt, it, state, GRADCLIP[L])
            rec.append((loss, norm, {n: p.detach().clone() for n, p in m.state_dict().items()}))
        runs[dtype] = rec
    ppl = {}
    for dtype in (torch.float32, torch.float64):
        m = ClassifierWithState(FSRNNLM(V, E, L, H, H, KEEP_H, KEEP_C))
        m.compute_accuracy = False
        m.load_state_dict(copy.deepcopy(lm.state_dict()))
        m = m.to(dtype)
        ppl[dtype] = evaluate(m, ParallelSequentialIterator(valid, BATCH, repeat=False), dtype)
    rec32, rec64 = runs[torch.float32], runs[torch.float64]
    coefs = [min(1.0, GRADCLIP[L] / (norm + 1e-6)) for _, norm, _ in rec32]
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), (coefs, [r[1] for r in rec32])
    worst = 0.0
    for (l32, n32, p32), (l64, n64, p64) in zip(rec32, rec64):
        worst = max([worst, abs(l32 - l64) / max(1.0, abs(l64))] + [rel(p32[n], p64[n]) for n in p32])
    worst = max(worst, abs(ppl[torch.float32] - ppl[torch.float64]) / ppl[torch.float64])
    assert worst <= QUARTER_BAR, 'fp32 is %.3e from fp64 over the three iterations: shrink the learning signal, not the bar' % worst
    for k, (loss, norm, params) in enumerate(rec32):
        fx[pre + 'train.it%d.loss' % k], fx[pre + 'train.it%d.norm' % k] = np.float64(loss), np.float64(norm)
        fx.update({pre + 'train.it%d.%s' % (k, n): p.numpy().copy() for n, p in params.items()})
    fx[pre + 'train.valid_ppl'] = np.float64(ppl[torch.float32])
    report.append('L%d: clip coefficients %s, fp32 vs fp64 %.2e (limit %.1e), validation perplexity %.6f'
                  % (L, [round(c, 4) for c in coefs], worst, QUARTER_BAR, ppl[torch.float32]))

    # ---- the predict chain ----------------------------------------------------------------------------------------------------------
    lm.eval()
    ids = np.asarray(CHAIN_IDS, np.int64)
    state, lps = None, []
    with torch.no_grad():
        for i in range(len(CHAIN_IDS)):
            if CHAIN_PARENTS[i] is not None:
                par = torch.tensor(CHAIN_PARENTS[i])
                state = {k: v.index_select(0, par) for k, v in state.items()}
            state, lp = lm.predict(state, torch.from_numpy(ids[i]))
            lps.append(lp.numpy().copy())
    fx[pre + 'chain.ids'] = ids
    fx[pre + 'chain.parents'] = np.asarray([p if p is not None else [0, 1, 2] for p in CHAIN_PARENTS], np.int64)
    fx[pre + 'chain.logp'] = np.stack(lps)
    for k, v in state.items():
        fx[pre + 'chain.' + k] = v.numpy().copy()
    return lm


def nbest(lm, fx, report):
    from model.e2e_model import E2E
    from model.feat_model import FbankModel
    opt = mf.tiny_opt()
    assert opt.odim == V
    torch.manual_seed(606)
    random.seed(0)
    asr = E2E(opt)
    fb = FbankModel(opt)
    clean, mix, mix_log, cos = mf.synth_batch(3, LENS, seed=11)
    cm = torch.stack([torch.linspace(10, 14, 80), torch.linspace(0.3, 0.6, 80)])
    feats = fb(clean, cm).detach()
    base = dict(np.load(os.path.join(HERE, 'recog_tiny.npz')))
    assert np.array_equal(base['feats'], feats.numpy()), 'not the model / utterances of recog_tiny.npz'
    lm.eval()
    fx['lens'], fx['lm_weights'] = np.array(LENS, np.int32), np.array(LM_WEIGHTS, np.float64)
    char_list = [str(i) for i in range(opt.odim)]
    gap = {w: np.inf for w in LM_WEIGHTS}
    for name, beam, penalty, ctcw, maxr, minr, nb in CONFIGS:
        for u, T in enumerate(LENS):
            args = argparse.Namespace(beam_size=beam, penalty=penalty, ctc_weight=ctcw, maxlenratio=maxr, minlenratio=minr, nbest=nb, lm_weight=0.0)
            with torch.no_grad():
                free = nbest_arrays(asr.recognize(feats[u:u + 1, :T], args, char_list))
            for w in LM_WEIGHTS:
                args.lm_weight = w
                with torch.no_grad():
                    seqs, scores = nbest_arrays(asr.recognize(feats[u:u + 1, :T], args, char_list, rnnlm=lm))
                assert seqs.shape != free[0].shape or not np.array_equal(seqs, free[0]), (name, u, w, 'n-best unchanged by the LM')
                if len(scores) > 1:
                    g = float(np.min(np.abs(np.diff(scores))))
                    assert g >= MIN_GAP, (name, u, w, g)
                    gap[w] = min(gap[w], g)
                fx['%s.%s.u%d.yseq' % (name, wtag(w), u)] = seqs
                fx['%s.%s.u%d.score' % (name, wtag(w), u)] = scores
    report.append('smallest adjacent-score gap: %s' % {w: float('%.3g' % g) for w, g in gap.items()})


def main():
    mf.install_shims()
    fx, report = {}, []
    # the L = 2 model decodes: the first seed whose LM changes every n-best list and leaves no two adjacent scores within MIN_GAP
    for seed in range(902, 942):
        lists = {}
        try:
            nbest(fresh_model(2, seed), lists, report)
        except AssertionError as e:
            print('seed %d: %s' % (seed, e))
            continue
        fx.update(lists)
        fx['L2.seed'] = np.int64(seed)
        break
    else:
        raise SystemExit('no seed gives n-best lists that all see the LM')
    one_model(2, seed, fx, report)
    one_model(3, 903, fx, report)
    np.savez_compressed(os.path.join(HERE, 'fsrnn_tiny.npz'), **fx)
    print('\n'.join(report))


if __name__ == '__main__':
    main()
