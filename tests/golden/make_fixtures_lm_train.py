#!/usr/bin/env python3
"""Golden vectors for training the language model (training side): the reference's own ClassifierWithState(RNNLM(11, 6, 10,
dropout_rate=0)) (model/lm.py:26-146) and ParallelSequentialIterator (data/lm_data_loader.py) on the CPU.

  win.*      one window of T = 4 steps x B = 3 rows from the zero state: per-step losses, the final state, the gradient of the summed
             loss with respect to all 11 parameters
  train.*    three iterations of the reference's loop body (lm.py:284-313: bproplen steps of the iterator, summed loss, zero_grad,
             backward, detach, clip_grad_norm_, SGD lr 1.0) on a 40-token corpus with batch 4 and bproplen 3: the loss, the gradient
             norm and the parameters after each iteration, then the validation perplexity of its evaluation loop (lm.py:240-272) on a
             16-token corpus.  GRADCLIP is chosen so that the clip coefficient is below 1 in at least one iteration and 1 in at least
             one (asserted); an fp64 run of the same three iterations must stay within 2.5e-4 of the fp32 one -- a quarter of the 1e-3
             parity bar the GPU tests hold the product to (asserted)
  cli.*      the defaults, option strings and types of lm_train.py's command line, as JSON
  iter.*     the iterator over (23 tokens, batch 4) for two epochs, with its counters after every step; the position at which a
             repeat=False iterator stops

Runs only where the reference can be imported; writes lm_train_tiny.npz.  No test imports this file."""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf   # noqa: E402

V, I, H = 11, 6, 10
WIN_T, WIN_B = 4, 3
CORPUS, VALID, BATCH, BPROPLEN, ITERS = 40, 16, 4, 3, 3
GRADCLIP = 1.2
QUARTER_BAR = 2.5e-4


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def loop_body(model, optimizer, it, state, clip_grad_norm_):
    """lm.py:285-313 for one iteration -> (state, loss, gradient norm before clipping)."""
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
    norm = clip_grad_norm_(model.parameters(), GRADCLIP)
    optimizer.step()
    return state, float(loss.detach()), float(norm)


def zero_state(dtype):
    """What ``state = None`` stands for (lm.py:133-139), in the run's dtype: the reference's own zeros are always fp32."""
    return {k: torch.zeros(BATCH, H, dtype=dtype) for k in ('c1', 'h1', 'c2', 'h2')}


def evaluate(model, it, dtype, bproplen=100):
    """lm.py:240-272."""
    torch.set_grad_enabled(False)
    model.predictor.eval()
    state, sum_perp, data_count = zero_state(dtype), 0, 0
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


def cli_table():
    """lm_train.py builds its parser inside main(): run main() with parse_args replaced by a recorder."""
    import lm_train
    seen = {}

    class Recorded(Exception):
        pass

    def record(self, *a, **kw):
        for act in self._actions:
            if act.dest != 'help':
                seen[act.dest] = dict(default=act.default, flags=sorted(act.option_strings), type=getattr(act.type, '__name__', None),
                                      required=bool(act.required))
        raise Recorded()

    orig = argparse.ArgumentParser.parse_args
    argparse.ArgumentParser.parse_args = record
    try:
        lm_train.main()
    except Recorded:
        pass
    finally:
        argparse.ArgumentParser.parse_args = orig
    assert len(seen) >= 20
    return seen


def main():
    mf.install_shims()
    from model.lm import ClassifierWithState, RNNLM
    from data.lm_data_loader import ParallelSequentialIterator
    torch.manual_seed(808)
    lm = ClassifierWithState(RNNLM(V, I, H, dropout_rate=0))
    lm.compute_accuracy = False
    for prm in lm.parameters():
        prm.data.uniform_(-1.0, 1.0)
    lm.train()
    fx = dict(mf.sd_np('lm.', lm))
    assert len(fx) == 11
    rng = np.random.RandomState(5)

    # ---- one window -------------------------------------------------------------------------------------------------------------
    xs, ts = rng.randint(0, V, (WIN_T, WIN_B)), rng.randint(0, V, (WIN_T, WIN_B))
    state, losses = None, []
    for t in range(WIN_T):
        state, loss = lm(state, torch.from_numpy(xs[t]).long(), torch.from_numpy(ts[t]).long())
        losses.append(loss)
    lm.zero_grad()
    sum(losses).backward()
    fx.update({'win.xs': xs.astype(np.int32), 'win.ts': ts.astype(np.int32), 'win.losses': np.array([float(v.detach()) for v in losses], np.float64)})
    fx.update({'win.state.' + k: v.detach().numpy().copy() for k, v in state.items()})
    fx.update(mf.grads_np('win.grad.', lm))
    assert sum(k.startswith('win.grad.') for k in fx) == 11

    # ---- three training iterations, in fp32 and in fp64 -------------------------------------------------------------------------
    corpus, valid = rng.randint(0, V, CORPUS).astype(np.int32), rng.randint(0, V, VALID).astype(np.int32)
    fx.update({'train.corpus': corpus, 'train.valid': valid, 'train.gradclip': np.float64(GRADCLIP)})
    runs = {}
    for dtype in (torch.float32, torch.float64):
        m = ClassifierWithState(RNNLM(V, I, H, dropout_rate=0))
        m.compute_accuracy = False
        m.load_state_dict(copy.deepcopy(lm.state_dict()))
        m = m.to(dtype).train()
        opt = torch.optim.SGD(m.parameters(), lr=1.0)
        it = ParallelSequentialIterator(corpus, BATCH)
        state, rec = zero_state(dtype), []
        for k in range(ITERS):
            state, loss, norm = loop_body(m, opt, it, state, torch.nn.utils.clip_grad_norm_)
            rec.append((loss, norm, {n: p.detach().clone() for n, p in m.state_dict().items()}))
        runs[dtype] = (rec, evaluate(m, ParallelSequentialIterator(valid, BATCH, repeat=False), dtype))
    rec32, ppl32 = runs[torch.float32]
    rec64, ppl64 = runs[torch.float64]
    coefs = [min(1.0, GRADCLIP / (norm + 1e-6)) for _, norm, _ in rec32]
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), coefs
    worst = 0.0
    for (l32, n32, p32), (l64, n64, p64) in zip(rec32, rec64):
        worst = max([worst, abs(l32 - l64) / max(1.0, abs(l64))] + [rel(p32[n], p64[n]) for n in p32])
    worst = max(worst, abs(ppl32 - ppl64) / ppl64)
    assert worst <= QUARTER_BAR, 'fp32 is %.3e from fp64 over the three iterations: shrink the learning signal, not the bar' % worst
    for k, (loss, norm, params) in enumerate(rec32):
        fx['train.it%d.loss' % k], fx['train.it%d.norm' % k] = np.float64(loss), np.float64(norm)
        fx.update({'train.it%d.%s' % (k, n): p.numpy().copy() for n, p in params.items()})
    fx['train.valid_ppl'] = np.float64(ppl32)

    # ---- the iterator -----------------------------------------------------------------------------------------------------------
    data = (np.arange(23) * 7 % 23).astype(np.int32)
    it = ParallelSequentialIterator(data, 4)
    batches, counters = [], []
    while it.epoch < 2:
        batches.append(np.array(it.__next__()))
        counters.append([it.iteration, it.epoch, int(it.is_new_epoch), it.epoch_detail, it.previous_epoch_detail])
    fx.update({'iter.data': data, 'iter.offsets': np.array(it.offsets, np.int64), 'iter.batches': np.stack(batches).astype(np.int32),
               'iter.counters': np.array(counters, np.float64)})
    it = ParallelSequentialIterator(data, 4, repeat=False)
    n = 0
    try:
        while True:
            it.__next__()
            n += 1
    except StopIteration:
        pass
    fx.update({'iter.stop_after': np.int64(n), 'iter.iteration_after_stop': np.int64(it.iteration), 'iter.epoch_after_stop': np.int64(it.epoch)})
    fx['cli.table'] = np.array(json.dumps(cli_table(), sort_keys=True))
    np.savez_compressed(os.path.join(HERE, 'lm_train_tiny.npz'), **fx)
    print('clip coefficients:', [round(c, 4) for c in coefs], ' norms:', [round(r[1], 4) for r in rec32], ' losses:', [round(r[0], 4) for r in rec32])
    print('fp32 vs fp64 over the three iterations: %.2e (limit %.1e)   validation perplexity %.6f' % (worst, QUARTER_BAR, ppl32))
    print('iterator: %d steps to epoch 2; repeat=False stops after %d steps' % (len(batches), n))


if __name__ == '__main__':
    main()
