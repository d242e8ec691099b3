#!/usr/bin/env python3
"""The FS-RNN LM: milliseconds per truncated-BPTT training window with the recurrence on the fused cell-step kernels of csrc/fsrnn.hip and on
the composed sequence (model/lm.py COMPOSED_PATH: re2e_gemm x 2 + re2e_lstm_cell_fwd / _bwd + element-wise blends per cell step), and
microseconds per output position of the LM at decode time, few-row kernels (re2e_lm_lstm_cell_zo) against the composed path.

The recipe's shape (train_fsrnnlm_2layer_256_650_drop0.5_bs64): E = 256, F = S = 650, fast_layers = 2, V = 4233, T = 35, dropout 0.5, keeps
0.9 / 0.5, at B = 64 and B = 2048.  One iteration = what model/fsrnn.py train() does per window: forward_seq, zero_grad, backward, detach,
clip at 5, SGD step.  Before any timing the two arms run the same window from the same parameters with the same masks and their losses and
gradients are compared (1e-4 / 2e-4 of the max).  Then the arms alternate ``--rounds`` times in one process after ``--warmup`` iterations
each; an iteration is timed with device events.

    python tools/bench_fsrnn.py                                 # both tables, then the kernel trace of one fused run (rocprofv3, a child process)
    python tools/bench_fsrnn.py --no-trace                      # the tables only
    python tools/bench_fsrnn.py --arm fused --batch 64          # a few iterations of one arm (what the trace runs)
    python tools/bench_fsrnn.py --kernel-stats DIR              # share of the two step kernels from a trace directory"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, E, H, V, L = 35, 256, 650, 4233, 2
KEEP_H, KEEP_C, DROPOUT = 0.9, 0.5, 0.5
TRACE_ITERS = 4                   # iterations of an --arm run (the first is the warm-up)


def kernel_stats(path):
    files = glob.glob(os.path.join(path, '**', '*kernel_stats.csv'), recursive=True) if os.path.isdir(path) else [path]
    assert files, 'no *kernel_stats.csv under %s' % path
    rows = list(csv.DictReader(open(files[0])))
    total = sum(float(r['TotalDurationNs']) for r in rows)
    for name in ('fsrnn_fwd_step', 'fsrnn_bwd_step'):
        sel = [r for r in rows if name in r['Name']]
        ns, calls = sum(float(r['TotalDurationNs']) for r in sel), sum(int(r['Calls']) for r in sel)
        print('%-16s calls %5d  average %8.2f us  %5.1f %% of kernel time' % (name, calls, ns / max(calls, 1) / 1e3, 100 * ns / total))
    print('ten largest kernels of the trace:')
    for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs']))[:10]:
        print('  %5.1f %%  calls %5d  average %9.2f us  %s' % (100 * float(r['TotalDurationNs']) / total, int(r['Calls']), float(r['AverageNs']) / 1e3, r['Name'][:90]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 2048])
    ap.add_argument('--beams', type=int, nargs='+', default=[12, 30])
    ap.add_argument('--batch', type=int, default=64, help='with --arm: the batch size')
    ap.add_argument('--rounds', type=int, default=9, help='alternations of the two arms')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--positions', type=int, default=50, help='output positions per timed decode run')
    ap.add_argument('--arm', choices=('fused', 'composed'), default=None, help='run only this arm, %d iterations (for a kernel trace)' % TRACE_ITERS)
    ap.add_argument('--kernel-stats', default=None)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--trace-dir', default=None, help='where rocprofv3 writes its trace (default: a fresh temporary directory)')
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats)

    import numpy as np
    import torch
    from robust_e2e_gan_amd import lib, ops
    from robust_e2e_gan_amd.model import lm as lm_mod
    from robust_e2e_gan_amd.model.fsrnn import FSRNNLM
    from robust_e2e_gan_amd.optim import FlatOptimizer
    assert torch.cuda.is_available() and lib.query('re2e_device_ok') == 1, 'needs an MI355X: there is nothing to measure on a CPU'
    dev = 'cuda:0'

    def make(seed=3, train=True):
        torch.manual_seed(seed)
        m = lm_mod.ClassifierWithState(FSRNNLM(V, E, L, H, H, KEEP_H, KEEP_C, dropout_rate=DROPOUT))
        m.compute_accuracy = False
        m = m.to(dev)
        return m.train() if train else m.eval()

    def window(B, seed):
        rng = np.random.RandomState(seed)
        return rng.randint(0, V, (T, B)).astype(np.int32), rng.randint(0, V, (T, B)).astype(np.int32)

    class Arm(object):
        def __init__(self, composed, B):
            self.composed, self.B = composed, B
            self.model = make()
            self.opt = FlatOptimizer(self.model.parameters(), kind='sgd', lr=1.0)
            self.state = None
            self.n = 0

        def iteration(self):
            xs, ts = window(self.B, 100 + self.n)
            self.n += 1
            lm_mod.COMPOSED_PATH = self.composed
            try:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                self.state, loss = self.model.forward_seq(self.state, xs, ts)
                self.opt.zero_grad()
                loss.backward()
                self.state = {k: v.detach() for k, v in self.state.items()}
                self.opt.clip_grad_norm(5.0)
                self.opt.step()
                t1.record()
                t1.synchronize()
                return t0.elapsed_time(t1), float(loss.detach())
            finally:
                lm_mod.COMPOSED_PATH = False

    if a.arm:
        arm = Arm(a.arm == 'composed', a.batch)
        for _ in range(TRACE_ITERS):
            arm.iteration()
        return

    def rel(x, y):
        return float((x.double() - y.double()).abs().max() / max(float(y.double().abs().max()), 1e-30))

    def table(ms, unit, per):
        print('  %-10s %14s %9s %9s %15s' % ('arm', 'median ' + unit, 'min', 'max', 'quartiles'))
        med, iqr = {}, {}
        for name, v in ms.items():
            q = statistics.quantiles(v, n=4)
            med[name], iqr[name] = statistics.median(v), q[2] - q[0]
            print('  %-10s %14.2f %9.2f %9.2f %7.2f-%-7.2f' % (name, med[name], min(v), max(v), q[0], q[2]))
        d, spread = med['composed'] - med['fused'], max(iqr.values())
        print('  fused is %.2f %s per %s %s than composed (%.2fx) against a spread of %.2f (widest interquartile range) -> %s'
              % (abs(d), unit, per, 'faster' if d > 0 else 'slower', med['composed'] / med['fused'], spread,
                 'separated' if abs(d) > spread else 'NOT separated from the spread'))

    print('FS-RNN LM: T = %d, E = %d, F = S = %d, fast_layers = %d, V = %d, dropout %.1f, keeps %.1f / %.1f; %s'
          % (T, E, H, L, V, DROPOUT, KEEP_H, KEEP_C, torch.cuda.get_device_name(0)))
    for B in a.batches:
        for backward in (False, True):
            print('plan B=%d %s: %s' % (B, 'bwd' if backward else 'fwd', ' '.join('%s=%s' % kv for kv in lib.fsrnn_plan(T, B, H, L, backward=backward).items())))
        print('masks of one window at B=%d: one (T,B,H) fp32 mask is %.1f MB, the window holds %d of them' % (B, T * B * H * 4 / 1e6, 2 * (L + 1) + 2))
        got = []
        for composed in (False, True):
            m = make()
            lm_mod.COMPOSED_PATH = composed
            ops.dropout_seed(5, 0)
            state, l0 = m.forward_seq(None, *window(B, 7))
            state, l1 = m.forward_seq({k: v.detach() for k, v in state.items()}, *window(B, 8))
            m.zero_grad()
            l1.backward()
            lm_mod.COMPOSED_PATH = False
            got.append((l1.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}))
        worst = max(rel(got[0][1][k], got[1][1][k]) for k in got[0][1])
        print('B=%d fused vs composed: loss %.2e, worst gradient %.2e of the max' % (B, rel(got[0][0], got[1][0]), worst))
        assert rel(got[0][0], got[1][0]) <= 1e-4 and worst <= 2e-4, 'the arms disagree: nothing to time'
        del got, m, state
        arms = {'fused': Arm(False, B), 'composed': Arm(True, B)}
        for arm in arms.values():
            for _ in range(max(1, a.warmup)):
                arm.iteration()
        ms = {name: [] for name in arms}
        for _ in range(max(5, a.rounds)):
            for name, arm in arms.items():
                ms[name].append(arm.iteration()[0])
        print('training window, B=%d, %d alternations after %d warm-up iterations each' % (B, max(5, a.rounds), max(1, a.warmup)))
        table(ms, 'ms', 'window')
        del arms
        torch.cuda.empty_cache()

    # decode: one output position = predict_combined for `beam` rows (state gather included, as the search does it)
    m = make(train=False)
    for beam in a.beams:
        g = torch.Generator().manual_seed(beam)
        ids = [torch.randint(0, V, (beam,), generator=g).to(dev) for _ in range(a.positions)]
        par = torch.randint(0, beam, (beam,), generator=g).to(dev)
        att = torch.randn(beam, V, generator=g).to(dev)

        def run(composed):
            lm_mod.COMPOSED_PATH = composed
            try:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                state = None
                t0.record()
                with torch.no_grad():
                    for x in ids:
                        if state is not None:
                            state = {k: v.index_select(0, par) for k, v in state.items()}
                        state, lp, comb = m.predict_combined(state, x, att, 0.2)
                t1.record()
                t1.synchronize()
                return t0.elapsed_time(t1) * 1e3 / len(ids), lp
            finally:
                lm_mod.COMPOSED_PATH = False
        lp_f, lp_c = run(False)[1], run(True)[1]
        assert rel(lp_f, lp_c) <= 2e-4, 'the decode arms disagree: nothing to time'
        us = {'fused': [], 'composed': []}
        for _ in range(max(1, a.warmup)):
            run(False), run(True)
        for _ in range(max(5, a.rounds)):
            us['fused'].append(run(False)[0])
            us['composed'].append(run(True)[0])
        print('decode, beam %d: us per output position over %d positions, %d alternations' % (beam, a.positions, max(5, a.rounds)))
        table(us, 'us', 'position')
    if not a.no_trace:
        B = a.batches[0]
        trace_dir = a.trace_dir or tempfile.mkdtemp(prefix='fsrnn_trace_')
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', trace_dir, '--', sys.executable, os.path.abspath(__file__),
               '--arm', 'fused', '--batch', str(B)]
        print('kernel trace (B=%d, %d iterations of the fused arm): %s' % (B, TRACE_ITERS, ' '.join(cmd[:8])))
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        kernel_stats(trace_dir)


if __name__ == '__main__':
    main()
