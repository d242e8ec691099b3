#!/usr/bin/env python3
"""SpecAugment on the device (csrc/specaug.hip re2e_spec_augment_fwd / _bwd through ops.spec_augment) measured on one MI355X:

  1  the two kernels alone at (32, 800, 80) with plans drawn for ESPnet's defaults '5,30,2,40,2' (ragged lengths), event timing on one
     stream, and the bytes per second they move (the tensor read once and written once; 16 MB fit the last-level cache, so the rate is
     not to be read as an HBM rate).  Their yardstick is MEASURED in the same process: a device-to-device copy of the same tensor
  2  the AsrTrainer step (BASELINE configuration 2) and the joint step (configuration 4) with and without ``spec_augment``, on ONE trainer
     whose option is switched round by round, so both arms share the process, the weights' shapes, the streams and the allocator

All arms of a section run in one process, alternated round by round; the tables give the median over the rounds and the (min .. max)
spread.  The result goes between the markers of profiles/spec_augment.md; what stands outside them is kept.
    python tools/bench_spec_augment.py [--rounds 5] [--steps 10] [--no-step] [--out profiles/spec_augment.md]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from robust_e2e_gan_amd import lib
from robust_e2e_gan_amd.data import spec_augment as sa

DEV = 'cuda:0'
CFG = '5,30,2,40,2'
R, TP, F = 32, 800, 80
BEGIN, END = '<!-- bench_spec_augment: begin -->', '<!-- bench_spec_augment: end -->'


def spread(xs):
    return '%.3f (%.3f .. %.3f)' % (statistics.median(xs), min(xs), max(xs))


def event_ms(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def write_between_markers(path, body):
    old = open(path).read() if os.path.exists(path) else ''
    if BEGIN in old and END in old:
        head, tail = old.split(BEGIN)[0], old.split(END)[1]
    else:
        head, tail = old, ''
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, 'w').write(head + BEGIN + '\n' + body + '\n' + END + tail)


def time_steps(step, tr, cfg, rounds, steps, warm=3):
    """ms per step of the two arms, the trainer's option switched round by round (round 0 warms both up)."""
    out = {'without spec_augment': [], "with spec_augment '%s'" % CFG: []}
    for r in range(rounds + 1):
        for k, c in zip(out, (None, cfg)):
            tr.spec_augment = c
            for _ in range(warm if r == 0 else 1):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            if r > 0:
                out[k].append((time.perf_counter() - t0) * 1e3 / steps)
    tr.spec_augment = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'spec_augment.md'))
    ap.add_argument('--no-step', action='store_true', help='section 1 only')
    a = ap.parse_args()
    assert lib.query('re2e_device_ok') == 1, 'not a gfx950 device'
    ft, bt = lib.query('re2e_spec_augment_geometry', 0), lib.query('re2e_spec_augment_geometry', 1)
    lines = ['# SpecAugment on one MI355X (tools/bench_spec_augment.py)', '',
             'Milliseconds, median (min .. max) over %d rounds, arms alternated round by round.  The kernels give a workgroup %d output frames '
             '(forward) and %d source frames (backward) of one row.' % (a.rounds, ft, bt), '']

    # ---- 1: the kernels alone, and a device-to-device copy as their yardstick ------------------------------------------------------------------
    lens = [TP - 23 * (b % 9) - b for b in range(R)]
    plan = sa.draw_plan(4, 17, 0, lens, F, CFG)
    pd = torch.from_numpy(plan).to(DEV)
    x = torch.randn(R, TP, F, device=DEV)
    y, g, dx = torch.empty_like(x), torch.randn(R, TP, F, device=DEV), torch.empty_like(x)
    arms = {'re2e_spec_augment_fwd': lambda: lib.call('re2e_spec_augment_fwd', x.data_ptr(), pd.data_ptr(), R, TP, F, 2, 2, y.data_ptr()),
            're2e_spec_augment_bwd': lambda: lib.call('re2e_spec_augment_bwd', g.data_ptr(), pd.data_ptr(), R, TP, F, 2, 2, dx.data_ptr()),
            'device-to-device copy of the tensor': lambda: y.copy_(x)}
    res = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            res[k].append(event_ms(fn))
    moved = 2.0 * x.numel() * 4
    lines += ['## 1: the kernels alone at (%d, %d, %d), plans drawn for %r over lengths %d .. %d' % (R, TP, F, CFG, min(lens), max(lens)), '',
              '| kernel | ms | MB moved (read once + written once) | GB/s (16 MB fit the last-level cache: not to be read as an HBM rate)  |', '|---|---|---|---|']
    for k, v in res.items():
        ms = statistics.median(v)
        lines.append('| %s | %s | %.1f | %.0f |' % (k, spread(v), moved / 1e6, moved / ms / 1e6))
    lines += ['', 'The copy row is the expectation the kernels are read against: a measured rate of this device for this tensor in this process, not a '
              'derived one.  (The warped frames read up to four source frames each; neighbours share them through the caches.)', '']

    # ---- 2: the training steps, with and without ------------------------------------------------------------------------------------------------
    if not a.no_step:
        import bench
        from robust_e2e_gan_amd.data.synthetic import make_batch
        from robust_e2e_gan_amd.joint_train import config4_opt
        from robust_e2e_gan_amd.model.e2e_model import E2E
        from robust_e2e_gan_amd.model.feat_model import FbankModel
        cfg = sa.parse(CFG)
        dev = torch.device(DEV)
        for cfg_id, title in ((2, 'AsrTrainer.step'), (4, 'JointTrainer.step')):
            opt = config4_opt()
            B, T, L = bench.CONFIG_SHAPES[cfg_id]
            batch = make_batch(B, T, L, opt.odim, seed=1234)
            cmvn_batches = [make_batch(B, T, L, opt.odim, seed=77 + i) for i in range(2)]
            if cfg_id == 2:
                torch.manual_seed(1234)
                enh, gan, fb, asr = None, None, FbankModel(opt).to(dev).train(), E2E(opt).to(dev).train()
                with torch.no_grad():
                    f = torch.cat([fb(b[0].to(dev))[i, :l] for b in cmvn_batches for i, l in enumerate(b[4].tolist())], 0)
                    cmvn = torch.stack([-f.mean(0), 1.0 / f.std(0)]).cpu()
            else:
                enh, fb, asr, gan = bench.build(opt, dev)
                cmvn = bench.synthetic_cmvn(enh, fb, cmvn_batches, dev)
            step, tr, _ = bench.make_stepper(cfg_id, opt, (enh, fb, asr, gan), batch, cmvn.to(dev), dev)
            ms = time_steps(step, tr, cfg, a.rounds, a.steps)
            base = statistics.median(ms['without spec_augment'])
            lines += ['## 2.%d: %s (configuration %d networks, B = %d, T = %d, %d labels), %d steps per round' % (1 if cfg_id == 2 else 2, title, cfg_id, B, T, L,
                                                                                                               a.steps), '',
                      '| arm | ms per step | minus the un-augmented arm (medians) |', '|---|---|---|']
            for k, v in ms.items():
                lines.append('| %s | %s | %+.3f |' % (k, spread(v), statistics.median(v) - base))
            lines.append('')
            del step, tr, enh, fb, asr, gan
            torch.cuda.empty_cache()
    else:
        lines += ['## 2: the training steps were NOT measured in this run (--no-step)', '']
    body = '\n'.join(lines)
    write_between_markers(a.out, body)
    print(body)


if __name__ == '__main__':
    main()
