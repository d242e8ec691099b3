#!/usr/bin/env python3
"""N-gram LMs in the beam search: what one position of the search costs on csrc/ngram.hip (re2e_ngram_step), against the host arbiter
(NgramTables.step_host: the per-row walk on the CPU plus the copies, what a host n-gram library costs at best) and against the RNNLM step
(model/lm.py), and what the LM adds to ``recognize`` end to end.  Writes profiles/recog_ngram.md.

The model is synthetic: every n-gram up to order 5 of a random label text over V = 4233 labels (labels drawn from a Zipf law, so contexts repeat
and successor lists have every length), with random log-probabilities and back-offs -- a suffix-closed model of roughly a million n-grams; the
exact count is printed.  Rows follow the text, so their states are as deep as a decoder's.

    python tools/bench_recog_ngram.py [--out profiles/recog_ngram.md]

Step arms, alternated ``--rounds`` times in one process after a warm-up: ``device`` (NgramLM.forward_combined: one launch, att + w * lp fused),
``host`` (the same through HOST_PATH), ``rnnlm`` (ClassifierWithState(RNNLM 256 / 650).predict_combined; above 64 rows that is its composed path).
A sample is ``--positions`` chained positions between two host clock reads with a device synchronisation before each: launch overhead and
the host's share are in it, as they are in a search."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V, ORDER = 4233, 5


def synthetic_tables(tokens, seed=3):
    """(tables, text): every n-gram up to ORDER of a Zipf label text of ``tokens`` labels, random values."""
    import numpy as np
    from robust_e2e_gan_amd.model.ngram import NgramTables
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, V + 1) ** 1.05
    text = rng.choice(V, size=tokens, p=p / p.sum()).astype(np.int64)
    text[::37] = V - 1                                              # sentence ends
    grams = [dict() for _ in range(ORDER)]
    for v in range(V):
        grams[0][(v,)] = None
    t = text.tolist()
    for i in range(len(t)):
        for k in range(2, min(ORDER, len(t) - i) + 1):
            grams[k - 1][tuple(t[i:i + k])] = None
    for k in range(ORDER):
        lp = -rng.uniform(0.05, 6.0, size=len(grams[k]))
        bo = -rng.uniform(0.0, 2.0, size=len(grams[k])) if k < ORDER - 1 else np.zeros(len(grams[k]))
        for g, a, b in zip(list(grams[k]), lp.tolist(), bo.tolist()):
            grams[k][g] = (a, b)
    return NgramTables.from_grams(grams, V, V - 1), text, [len(g) for g in grams]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tokens', type=int, default=310000, help='labels of the random text the model is counted from')
    ap.add_argument('--rows', type=int, nargs='+', default=[12, 30, 192])
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--positions', type=int, default=24)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'recog_ngram.md'))
    a = ap.parse_args()

    import numpy as np
    import torch
    from robust_e2e_gan_amd import lib
    from robust_e2e_gan_amd.joint_train import config4_opt
    from robust_e2e_gan_amd.model import lm as lm_mod, ngram
    from robust_e2e_gan_amd.model.e2e_model import E2E
    dev = 'cuda:0'
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say('# Beam search with an n-gram LM: what the language model costs per output position')
    say()
    say('One MI355X, one process.  A synthetic ARPA-style back-off model (every n-gram up to order %d of a random Zipf label text over V = %d labels, '
        'random values), as flat tables in HBM (`model/ngram.py`).  Three arms for the LM step -- `device`: `re2e_ngram_step` (`csrc/ngram.hip`), one '
        'launch that advances the rows, writes the (n, V) log-probabilities and `att + lm_weight * lp`; `host`: the same arithmetic in numpy on the host '
        'over the same arrays (`ngram.HOST_PATH`: one read-back of the states and labels, one upload of the scores per position -- what a host n-gram library '
        'costs at best); `rnnlm`: the RNNLM step (256 / 650 units; above 64 rows its composed path) -- alternated %d times after a warm-up.  A sample is %d '
        'chained positions whose rows follow the text (so their states are as deep as a decoder\'s), between two host clock reads with a device '
        'synchronisation before each: launch overhead and the host\'s share are in it, as in a search.  12 and 30 rows are `recognize` at those beams, '
        '192 rows `recognize_batch` of 16 utterances at beam 12.' % (ORDER, V, max(5, a.rounds), a.positions))
    say()
    say('    python tools/bench_recog_ngram.py')
    say()
    t0 = time.perf_counter()
    tables, text, sizes = synthetic_tables(a.tokens)
    built = time.perf_counter() - t0
    nlm = lm_mod.ClassifierWithState(ngram.NgramLM(tables)).to(dev).eval()
    torch.manual_seed(22)
    rnn = lm_mod.ClassifierWithState(lm_mod.RNNLM(V, 256, 650))
    rnn.predictor.lo.weight.data.uniform_(-0.5, 0.5)
    rnn = rnn.to(dev).eval()
    table_mb = sum(getattr(tables, n).nbytes for n in tables.ARRAYS) / 1e6
    say('model: order %d over V = %d labels, %d n-grams (%s by order), %d nodes, %d successor entries, %.1f MB of tables; built in %.1f s on the host'
        % (ORDER, V, sum(sizes), ' / '.join(map(str, sizes)), tables.n_nodes, tables.n_succ, table_mb, built))

    def chain_bytes(states):
        """Successor entries (label + log-probability, 8 bytes) the step streams for these new states, and the unigram rows."""
        total = 0
        for d in states.tolist():
            for nd in tables._chain(int(d))[0][:-1]:
                total += 8 * int(tables.succ_off[nd + 1] - tables.succ_off[nd])
            total += 4 * V
        return total

    def run(arm, n, starts, measure_bytes=False):
        """``--positions`` chained positions of n rows that follow the text from ``starts``; returns (us per position, bytes per position)."""
        model = rnn if arm == 'rnnlm' else nlm
        ngram.HOST_PATH = arm == 'host'
        att = torch.randn(n, V, device=dev)
        state, moved = None, 0
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for pos in range(a.positions):
                x = text[starts + pos].astype(np.int32)
                state, lp, comb = model.predict_combined(state, x, att, 0.3)
                if measure_bytes:
                    moved += chain_bytes(state['node'].cpu().numpy()) + 3 * n * V * 4          # lp and comb written, att read
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / a.positions, moved / a.positions
        finally:
            ngram.HOST_PATH = False

    def back_to_back(n, starts, launches=200):
        """us per launch of the device step alone: the same position ``launches`` times between two device events, no host work in between
        but the launch itself -- the kernel's duration, or the rate at which the host can issue it, whichever is longer."""
        state = None
        for pos in range(ORDER + 1):                               # reach deep states first
            state, _, _ = nlm.predict_combined(state, text[starts + pos].astype(np.int32), None, 0.0)
        pred, node = nlm.predictor, state['node']
        ids = torch.from_numpy(text[starts + ORDER + 1].astype(np.int32)).to(dev)
        att = torch.randn(n, V, device=dev)
        new, lp, comb = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, V, device=dev), torch.empty(n, V, device=dev)
        targs = tables.table_args({name: getattr(pred, name) for name in tables.ARRAYS})
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = None
        for _ in range(5):
            e0.record()
            for _ in range(launches):
                lib.call('re2e_ngram_step', *targs, node.data_ptr(), ids.data_ptr(), n, att.data_ptr(), 0.3, new.data_ptr(), lp.data_ptr(), comb.data_ptr())
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1) * 1e3 / launches
            best = t if best is None else min(best, t)
        return best

    arms = ('device', 'host', 'rnnlm')
    rng = np.random.default_rng(0)
    say()
    say('## One position of the search: the LM step alone')
    say()
    say('```')
    say('%5s  %-7s %14s %10s %10s %14s' % ('rows', 'arm', 'median us/pos', 'min', 'max', 'quartiles'))
    summary = []
    for n in a.rows:
        starts = rng.integers(0, len(text) - a.positions - 1, size=n)
        _, moved = run('device', n, starts, measure_bytes=True)
        for arm in arms:
            run(arm, n, starts)                                    # warm-up
        samples = {arm: [] for arm in arms}
        for _ in range(max(5, a.rounds)):
            for arm in arms:
                samples[arm].append(run(arm, n, starts)[0])
        med = {}
        for arm in arms:
            v = samples[arm]
            q = statistics.quantiles(v, n=4)
            med[arm] = statistics.median(v)
            say('%5d  %-7s %14.1f %10.1f %10.1f %6.1f-%-7.1f' % (n, arm, med[arm], min(v), max(v), q[0], q[2]))
        summary.append((n, med, moved, back_to_back(n, starts)))
    say('```')
    say()
    say('Bytes a device step must move -- n x V x 4 of lp written, the same of comb written and of att read, the unigram row and the successor '
        'entries (8 bytes each) of every level of every row\'s chain -- against the time of the step:')
    say()
    say('```')
    say('%5s %16s %18s %16s %18s %14s' % ('rows', 'bytes/position', 'of that successors', 'GB/s in a search', 'us back to back', 'GB/s at that'))
    for n, med, moved, b2b in summary:
        say('%5d %16d %18d %16.1f %18.2f %14.1f' % (n, moved, moved - 4 * n * V * 4, moved / med['device'] / 1e3, b2b, moved / b2b / 1e3))
    say('```')
    say()
    say('"us back to back": the same launch 200 times between two device events (best of five), nothing else on the host -- the kernel\'s duration or '
        'the rate at which the host can issue it, whichever is longer.  The step in a search (first table) is that plus the upload of the labels and the '
        'host side of a position.  Against the chip\'s HBM rate (8 TB/s) the step is nowhere near the bytes it moves at 12 and 30 rows: it is one short '
        'launch whose length is set by the dependent loads of the chain walk, not by bandwidth.')
    for n, med, moved, b2b in summary:
        say('* %d rows: device %.1f us, host path %.1f us (%.1fx), RNNLM step %.1f us (%.1fx).'
            % (n, med['device'], med['host'], med['host'] / med['device'], med['rnnlm'], med['rnnlm'] / med['device']))

    # ---- recognize end to end -------------------------------------------------------------------------------------------------------------------
    opt = config4_opt()
    torch.manual_seed(21)
    asr = E2E(opt).to(dev).eval()
    feats = torch.randn(1, 800, 80, generator=torch.Generator().manual_seed(4)).to(dev)
    with torch.no_grad():
        hpad, _ = asr.enc(feats, [800])
        lpz = asr.ctc.log_softmax(hpad)[0]
    h = hpad[0]

    def search(arm, beam):
        args = argparse.Namespace(beam_size=beam, penalty=0.0, ctc_weight=0.3, maxlenratio=0.25, minlenratio=0.0, nbest=1, lm_weight=0.2)
        ngram.HOST_PATH = arm == 'host'
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            asr.dec.recognize_beam(h, lpz, args, opt.char_list, rnnlm={'none': None, 'device': nlm, 'host': nlm, 'rnnlm': rnn}[arm])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / 50           # maxlenratio 0.25 x 200 frames = 50 positions
        finally:
            ngram.HOST_PATH = False

    say()
    say('## `recognize` end to end: 200 encoder frames, 50 positions, ctc_weight 0.3, lm_weight 0.2')
    say()
    say('```')
    say('%5s  %-7s %14s %10s %10s %14s' % ('beam', 'arm', 'median us/pos', 'min', 'max', 'quartiles'))
    sarms = ('none', 'device', 'host', 'rnnlm')
    costs = []
    for beam in (12, 30):
        for arm in sarms:
            search(arm, beam)
        samples = {arm: [] for arm in sarms}
        for _ in range(max(5, a.rounds)):
            for arm in sarms:
                samples[arm].append(search(arm, beam))
        for arm in sarms:
            v = samples[arm]
            q = statistics.quantiles(v, n=4)
            say('%5d  %-7s %14.1f %10.1f %10.1f %6.1f-%-7.1f' % (beam, arm, statistics.median(v), min(v), max(v), q[0], q[2]))
        m = {arm: statistics.median(samples[arm]) for arm in sarms}
        iqr = max(statistics.quantiles(samples[arm], n=4)[2] - statistics.quantiles(samples[arm], n=4)[0] for arm in sarms)
        costs.append('* beam %d: the LM adds %.1f us per position on the device step, %.1f us on the host path, %.1f us as an RNNLM (arm - none; widest '
                     'interquartile range of an arm %.1f us).' % (beam, m['device'] - m['none'], m['host'] - m['none'], m['rnnlm'] - m['none'], iqr))
    say('```')
    say()
    for line in costs:
        say(line)
    say()
    say('## Not measured')
    say()
    say('* The kernel under a profiler (its duration apart from the launch), and no hardware counters: the statement that the chain walk bounds the '
        'step rests on the byte counts above and on the kernel\'s structure, not on an attribution.')
    say('* A model estimated from text (real successor-list lengths and back-off depths differ from this synthetic one), orders above 5, and '
        '`recognize_batch` end to end: 192 rows are measured as the step alone.')
    say('* The table build (host, once per model; printed above) against reading the `.npz` cache.')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
