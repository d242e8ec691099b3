#!/usr/bin/env python3
"""joint_train step throughput on N MI355X (BASELINE.json metric), one process per GPU.

    python bench.py --gpus 1 --steps 10 --warmup 3
    python bench.py --gpus 1 --steps 10 --warmup 3 --dump-outputs DIR   # + what the last timed step computed: DIR/<name>.npy
    python bench.py --gpus 1 --steps 10 --warmup 3 --full               # + every measurement and check beside the headline (below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
    python bench.py --gpus N ...        # N > 1 without WORLD_SIZE in the environment: spawns the line above itself
                                        # (fresh child processes, started before this process touches a GPU)

A "step" is one full joint_train.py:156-212 iteration (enhancer -> fbank -> shared E2E (+CTC,
+location-attention decoder) -> CORAL -> discriminator; G-step and D-step; backward, clip, Adadelta)
on one synthetic AISHELL-shaped batch (config 4: B=32 per GPU, T=800, F=257->80, L=40, V=4233)
that is already resident in HBM.  Weak scaling: every rank processes its own B=32 batch and the
flat gradient buffers are averaged with RCCL.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line: metric, value, unit, ms_per_step, the
configuration, the final losses, and the gates that need no run of their own (no persistent-kernel aborts, finite losses and, with
N > 1, identical replicas).  Everything that needs runs of its own is --full only, where the --no-* options can drop parts of it:
the extra untimed steps (FLOP meter -> step_executed_*, the all-reduce timeline -> comm_timeline with N > 1), the second timed loop fed
from host memory (input_side) and the objects below.  The warm-up steps are the same with and without --full.

Extra objects on the line (--full):
  roofline     -- the dominant convolution (3x3 at the VGG conv1_2 shape of this workload, as the step launches it:
                  fused Winograd + ReLU + pool) timed live with HIP events on the launch stream; achieved / frac = EXECUTED
                  matrix-core FLOPs against the fp32-MFMA peak (<= 1), the direct-form figure is direct_equivalent_tflops
  roofline_engine -- the fp32-MFMA engine measured live: the heaviest GEMM / convolution rows of one step, each timed alone with HIP events and
                  weighted by its calls per step: executed TFLOP/s, fraction of the 157.3 peak, ms per step
  roofline_chain -- the latency-bound recurrent chains: us per step of the persistent bi-LSTM kernels alone on the chip, measured
                  live, next to the bare hand-off floor (tools/micro/handoff_probe.hip) and the MFMA floor
  other_configs -- configurations 2, 3 and 5 of BASELINE.json, 10 timed steps each in this same process (N = 1, --config 4)
  cpu_baseline -- the CPU oracle (oracle/joint.py, "port") timed on this box's host cores on the metric's own configuration
                  (rank 0, N=1 only): B=32, 1 warm-up (the parity step) + 3 timed steps, median; a B=8 sample next to it
  parity       -- the FIRST GPU step against the oracle's step on the SAME full batch, initial weights and cmvn
                  (relative errors of the losses, the clipped-gradient norm and enhance_out); the bench FAILS
                  if any exceeds 1e-3 (north_star's fp32 bar, SURVEY 8d "parity gate in the same run")
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3          # MI355X_MICROARCH.md, 'Peak FP32 (matrix)'
FLOP_PER_UTT = {2: 41.45e9, 3: 60.71e9, 4: 189.83e9, 5: 715.6e9}


def log(msg):
    if int(os.environ.get('RANK', '0')) == 0:
        print('[bench %7.1fs] %s' % (time.time() - _T0, msg), file=sys.stderr, flush=True)


_T0 = time.time()


def host_cores():
    """Usable host cores: scheduler affinity capped by the cgroup CPU quota (os.cpu_count() reports the whole machine)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        q, p = open('/sys/fs/cgroup/cpu.max').read().split()
        if q != 'max':
            n = min(n, max(1, int(float(q) / float(p))))
    except Exception:
        pass
    return max(1, min(n, 64))


def build(opt, dev):
    from robust_e2e_gan_amd.model.enhance_model import EnhanceModel
    from robust_e2e_gan_amd.model.feat_model import FbankModel
    from robust_e2e_gan_amd.model.e2e_model import ShareE2E
    from robust_e2e_gan_amd.model.gan_model import GANModel
    torch.manual_seed(1234)
    nets = [EnhanceModel(opt), FbankModel(opt), ShareE2E(opt), GANModel(opt)]
    return [m.to(dev).train() for m in nets]


def synthetic_cmvn(enh, fb, batches, dev):
    """F4: CMVN of the enhanced features over a few synthetic batches (feat_model.py:62-90)."""
    fb.cmvn_num = sum(int(b[4].numel()) for b in batches)
    out = None
    with torch.no_grad():
        for b in batches + batches[:1]:
            eo = enh(b[1].to(dev), b[2].to(dev), b[4])
            out = fb.compute_cmvn(eo, b[4])
    assert out is not None
    return torch.FloatTensor(out)


def _time_launches(fn, iters):
    """Average duration of ``iters`` back-to-back launches, HIP events on the launch stream."""
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def _profile_json(names):
    for n in names:
        try:
            return json.load(open(os.path.join(ROOT, 'profiles', n))), 'profiles/' + n
        except Exception:
            pass
    return None, None


def engine_average():
    """Average TFLOP/s of the fp32-MFMA engine over every GEMM / convolution call of one single-stream step, from the committed per-call
    table (tools/igemm_table.py over a RE2E_NO_OVERLAP=1 rocprofv3 kernel trace of this script): (direct-equivalent, executed, source).
    Direct-equivalent counts a Winograd call with the FLOPs of the direct convolution it replaces; executed is what the matrix cores did."""
    import re
    for n in ('r06_igemm_calls_nooverlap.txt', 'r05_igemm_calls_nooverlap.txt', 'r04_igemm_calls_nooverlap.txt', 'r03_igemm_calls_nooverlap.txt'):
        try:
            txt = open(os.path.join(ROOT, 'profiles', n)).read()
            m = re.search(r'total .*?([\d.]+) TFLOP/s average', txt)
            e = re.search(r'executed by the matrix cores: [\d.]+ TFLOP = ([\d.]+) TFLOP/s average', txt)
            if m:
                return float(m.group(1)), (float(e.group(1)) if e else None), 'profiles/' + n
        except Exception:
            pass
    return None, None, None


def conv_roofline(dev, iters=20):
    """Average launch duration of the dominant convolution, measured with HIP events on the stream the kernel is launched on: the 3x3
    convolution at the VGG conv1_2 shape of this workload (2B=64 images, 800x80, 64->64) AS THE TRAINING STEP LAUNCHES IT:
    ``re2e_conv3x3_wino`` with the fused ReLU + 2x2 max pool epilogue (csrc/winograd.hip: fused Winograd F(2x2,3x3), the input patch staged
    through LDS by LDS-DMA since round 6; only the pooled tensor and the index bytes are written).  Timed at the full height of the 64 images; the
    step launches it row-limited (``re2e_conv3x3_wino_rows``).

    ``achieved`` = the FLOPs the matrix cores EXECUTE per launch (the Winograd form: 16 instead of 36 multiply-adds per 2x2 outputs, i.e. the
    direct form's 2*9*Cin*Cout per output pixel / 2.25) / launch time, so ``frac`` <= 1 is a utilisation of the 157.3 TFLOP/s fp32-MFMA peak;
    the direct-form (SURVEY 8(d) algorithmic) figure, which can exceed the peak, is ``direct_equivalent_tflops``.  The direct kernels of the
    same product (round 2's halo-patch kernel, fused with the pool and plain) are timed next to it."""
    from robust_e2e_gan_amd import lib, ops
    N, H, W, C, K = 64, 800, 80, 64, 64
    x = torch.randn(N, H, W, C, device=dev)
    Wt = torch.randn(K, C, 3, 3, device=dev) * 0.04
    wg = torch.empty(K, 3, 3, C, device=dev)
    lib.call('re2e_conv_weight_gather', Wt.data_ptr(), wg.data_ptr(), K, C, 3, 3, 0, 3, 3, 0, 0, 1)
    b = torch.zeros(K, device=dev)
    y = torch.empty(N, H, W, K, device=dev)
    pooled = torch.empty(N, (H + 1) // 2, (W + 1) // 2, K, device=dev)
    idx = torch.empty(N, (H + 1) // 2, (W + 1) // 2, K, dtype=torch.uint8, device=dev)
    args = (x.data_ptr(), N, H, W, C, wg.data_ptr(), K, 3, 3, H, W, 1, 1, 1, 1, -1, -1, y.data_ptr(), H, W, 1, 1, 0, 0, b.data_ptr(),
            lib.ACT_RELU, 0.0)
    sec_wino = _time_launches(lambda: ops.conv3x3_wino(x, Wt, K, bias=b, relu=True, pool=True), iters)
    sec_plain = _time_launches(lambda: lib.call('re2e_conv_igemm', *args), iters)
    sec_pool = _time_launches(lambda: lib.call('re2e_conv3x3_relu_pool', x.data_ptr(), N, H, W, C, wg.data_ptr(), K, b.data_ptr(),
                                               pooled.data_ptr(), idx.data_ptr()), iters)
    flops = 2.0 * 9 * C * K * N * H * W                 # direct form
    exe = flops / 2.25                                  # what F(2x2,3x3) executes on the matrix cores: 16 instead of 36 multiply-adds per 2x2 outputs
    ach = exe / sec_wino / 1e12
    # HBM-side bytes per launch from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE on this same
    # kernel and shape, tools/roofline_conv.py); a counter pass cannot run inside this process.
    pj, tsrc = _profile_json(['r06_conv1_2_wino_pmc_traffic.json', 'r05_conv1_2_wino_pmc_traffic.json', 'r04_conv1_2_wino_pmc_traffic.json', 'r03_conv1_2_wino_pmc_traffic.json'])
    pj2, tsrc2 = _profile_json(['r03_conv1_2_pmc_traffic.json', 'r02_conv1_2_pmc_traffic.json'])
    eng, eng_exe, esrc = engine_average()
    pk = PEAK_FP32_MFMA_TFLOPS
    return {'bound': 'mfma', 'kernel': 'wino_conv3x3_kernel<8, LDSIN> (VGG conv1_2 forward: fused Winograd F(2x2,3x3) + bias + ReLU + 2x2 max pool in one launch, '
                                       '64x800x80, 64->64, 3x3, at its FULL height; the step launches the same kernel through re2e_conv3x3_wino_rows, '
                                       'which skips the 12-14 % of the rows beyond the utterances)',
            'achieved': round(ach, 2), 'peak': pk, 'unit': 'TFLOP/s', 'frac': round(ach / pk, 4),
            'note': 'achieved = EXECUTED matrix-core FLOPs (the Winograd form: direct FLOPs / 2.25) / launch time, so frac <= 1 is a utilisation of the '
                    'fp32-MFMA peak; the direct-form figure is direct_equivalent_tflops',
            'direct_equivalent_tflops': round(flops / sec_wino / 1e12, 2), 'algorithmic_speedup_vs_direct': 2.25,
            'traffic': pj['traffic_bytes_per_launch'] if pj else None,
            'traffic_unit': 'bytes per launch (FETCH_SIZE x2 + WRITE_SIZE)', 'traffic_source': tsrc,
            'algorithmic_bytes_per_launch': 4.0 * (N * H * W * C + 16 * K * C) + 5.0 * pooled.numel(),
            'avg_launch_ms': round(sec_wino * 1e3, 4), 'executed_flop_per_launch': exe, 'direct_flop_per_launch': flops,
            'direct_kernels': {
                'relu_pool': {'entry': 're2e_conv3x3_relu_pool (halo-patch direct kernel, fused pool)', 'avg_launch_ms': round(sec_pool * 1e3, 4),
                              'achieved': round(flops / sec_pool / 1e12, 2), 'frac': round(flops / sec_pool / 1e12 / pk, 4)},
                'plain': {'entry': 're2e_conv_igemm (halo-patch direct kernel, conv + bias + ReLU, full-resolution output)',
                          'avg_launch_ms': round(sec_plain * 1e3, 4), 'achieved': round(flops / sec_plain / 1e12, 2),
                          'frac': round(flops / sec_plain / 1e12 / pk, 4), 'traffic': pj2['traffic_bytes_per_launch'] if pj2 else None,
                          'traffic_source': tsrc2, 'algorithmic_bytes_per_launch': 4.0 * (N * H * W * C + N * H * W * K + K * 9 * C)}},
            'engine_avg_executed_tflops': eng_exe, 'engine_avg_executed_frac': round(eng_exe / pk, 4) if eng_exe else None,
            'engine_avg_direct_equivalent_tflops': eng, 'engine_avg_source': esrc,
            'engine_avg_note': 'per-call table of one single-stream step over every GEMM / convolution call; executed = matrix-core FLOPs, '
                               'direct-equivalent counts Winograd calls with the FLOPs of the direct convolution they replace',
            # what the committed SQ counter passes of THIS kernel say (read from the file, nothing modelled): matrix-pipe utilisation in shader
            # cycles, the clock the kernel really ran at (the 157.3 TFLOP/s peak assumes 2.4 GHz), vector instructions per MFMA
            'counters': _wino_counters()}


def _wino_counters():
    pj, src = _profile_json(['r06_conv1_2_wino_pmc_sq.json', 'r05_conv1_2_wino_pmc_sq.json'])
    if not pj:
        return None
    d = pj.get('derived', {})
    return {'source': src, 'mfma_pipe_utilisation': d.get('mfma_pipe_utilisation'), 'vector_instructions_per_mfma': d.get('other_vector_instructions_per_mfma'),
            'shader_clock_ghz': d.get('shader_clock_ghz'), 'wave_cycles_split': d.get('wave_cycles_split')}


def engine_roofline(dev, iters=8):
    """The fp32-MFMA engine's own roofline, measured LIVE: the heaviest GEMM / convolution calls of one config-4 step (the rows that make
    up >= 85 % of the per-call table profiles/r0N_igemm_calls_nooverlap.txt), each timed alone with HIP events on the launch stream and
    weighted by its calls per step.  ``executed_tflops`` = executed matrix-core FLOPs (Winograd rows: the FLOPs the transformed products
    really run, not the direct convolution's) / time; ``frac`` against the 157.3 TFLOP/s peak; ``ms_per_step`` = the rows' time per step."""
    from robust_e2e_gan_amd import lib, ops
    r = lambda *sh: torch.randn(*sh, device=dev)
    rows = []

    def add(name, calls, exe_flop, fn):
        sec = _time_launches(fn, iters)
        rows.append({'row': name, 'calls_per_step': calls, 'ms': round(sec * 1e3, 4), 'executed_tflops': round(exe_flop / sec / 1e12, 1)})
        return sec * calls, exe_flop * calls

    tot_s = tot_f = 0.0
    # dense x W^T (csrc/gemm_nt.hip) and dy^T x (csrc/igemm.hip): Linear forwards / input gradients, weight gradients
    for (M, N, K, calls) in ((12800, 2560, 2048, 2), (12288, 2048, 2560, 2), (12800, 512, 2048, 4), (12288, 2048, 512, 4), (24576, 1024, 512, 3),
                             (25600, 512, 1024, 2), (12800, 1024, 512, 3), (12800, 512, 1024, 3), (24576, 1024, 260, 3)):
        A, B, C = r(M, K), r(N, K), torch.empty(M, N, device=dev)
        t, f = add('x W^T %dx%dx%d' % (M, N, K), calls, 2.0 * M * N * K, lambda: ops.gemm(A, B, C, M, N, K, transb=True))
        tot_s, tot_f = tot_s + t, tot_f + f
    for (M, N, K, calls) in ((2048, 512, 12800, 10), (2048, 2560, 12800, 2), (1024, 256, 25600, 4), (1024, 512, 25600, 2), (512, 1024, 12800, 3)):
        A, B, C = r(K, M), r(K, N), torch.empty(M, N, device=dev)
        t, f = add('dy^T x %dx%dx%d' % (M, N, K), calls, 2.0 * M * N * K, lambda: ops.gemm(A, B, C, M, N, K, transa=True))
        tot_s, tot_f = tot_s + t, tot_f + f
    # discriminator 4x4 / stride-2 layers: forward and stride-2 data gradient (implicit GEMM on the same pipeline)
    for (Nb, H, W, C, Kc, cf, cd) in ((32, 400, 40, 64, 128, 3, 3), (32, 200, 20, 128, 256, 2, 2)):
        x, wt = r(Nb, H, W, C), r(Kc, C, 4, 4) * 0.05
        OH, OW = H // 2, W // 2
        wg = torch.empty(Kc, 4, 4, C, device=dev)
        lib.call('re2e_conv_weight_gather', wt.data_ptr(), wg.data_ptr(), Kc, C, 4, 4, 0, 4, 4, 0, 0, 1)
        y, dy = torch.empty(Nb, OH, OW, Kc, device=dev), r(Nb, OH, OW, Kc)
        fl = 2.0 * 16 * C * Kc * Nb * OH * OW
        t, f = add('D conv %d->%d 4x4/s2 fwd' % (C, Kc), cf, fl, lambda: lib.call('re2e_conv_igemm', x.data_ptr(), Nb, H, W, C, wg.data_ptr(), Kc, 4, 4, OH, OW, 2, 2,
                                                                                 1, 1, -1, -1, y.data_ptr(), OH, OW, 1, 1, 0, 0, None, lib.ACT_LRELU, 0.0))
        tot_s, tot_f = tot_s + t, tot_f + f
        t, f = add('D conv %d->%d 4x4/s2 dgrad' % (C, Kc), cd, fl, lambda: ops.conv_dgrad(dy, wt, (Nb, H, W, C), 2, 1))
        tot_s, tot_f = tot_s + t, tot_f + f
    # VGG 3x3 layers: fused Winograd forward + data gradient (executed = direct / 2.25)
    for (Nb, H, W, C, Kc) in ((64, 800, 80, 64, 64), (64, 400, 40, 64, 128), (64, 400, 40, 128, 128)):
        x, wt, dy = r(Nb, H, W, C), r(Kc, C, 3, 3) * 0.04, r(Nb, H, W, Kc)
        fl = 2.0 * 9 * C * Kc * Nb * H * W / 2.25
        t, f = add('VGG conv %d->%d 3x3 fwd (Winograd)' % (C, Kc), 1, fl, lambda: ops.conv3x3_wino(x, wt, Kc))
        tot_s, tot_f = tot_s + t, tot_f + f
        if C % 64 == 0:
            t, f = add('VGG conv %d->%d 3x3 dgrad (Winograd)' % (C, Kc), 1, fl, lambda: ops.conv3x3_wino(dy, wt, C, dgrad=True))
            tot_s, tot_f = tot_s + t, tot_f + f
        del x, dy
    ach = tot_f / tot_s / 1e12
    return {'bound': 'mfma', 'executed_tflops': round(ach, 1), 'peak': PEAK_FP32_MFMA_TFLOPS, 'frac': round(ach / PEAK_FP32_MFMA_TFLOPS, 4),
            'ms_per_step': round(tot_s * 1e3, 2), 'rows': rows,
            'note': 'each row alone on the chip, HIP events on the launch stream, %d launches after 3 warm-ups; weights = calls per config-4 step; the '
                    'Winograd / F(2x2,4x4) weight gradients and the small products are not in the list' % iters}


def chain_roofline(dev):
    """The recurrent chains' own roofline (they are latency-bound: neither HBM nor MFMA describes them).  Measured live: microseconds
    per step of the persistent bi-LSTM kernels alone on the chip at this workload's two shapes (enhancer 2 x 800 steps at H=256 / B=32,
    BLSTMP 3 x 200 steps at H=512 / B=64).  Floors: ``handoff_floor_us`` = the bare exchange of one step's state between the same
    number of workgroups with nothing computed (tools/micro/handoff_probe.hip, committed run profiles/r04_handoff_probe*.txt: a step
    cannot be shorter than the hand-off it contains); ``mfma_floor_us`` = the step's matrix FLOPs / (the CUs the chain runs on x their
    fp32-MFMA rate)."""
    from robust_e2e_gan_amd import lib
    out = {}
    floors = {(256, 32): {'fwd': 2.14, 'bwd': 3.12}, (512, 64): {'fwd': 3.02, 'bwd': 5.38}}      # profiles/r04_handoff_probe.txt (protos 1 / 5, 3)
    for name, T, B, H in (('enhancer_blstm_H256_B32', 800, 32, 256), ('blstmp_H512_B64', 200, 64, 512)):
        g = torch.Generator().manual_seed(T + B + H)
        xg0 = [(torch.randn(T * B, 4 * H, generator=g) * 0.5).to(dev) for _ in range(2)]
        whh = [(torch.randn(4 * H, H, generator=g) / H ** 0.5).to(dev) for _ in range(2)]
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        dy = (torch.randn(T * B, 2 * H, generator=g) * 0.3).to(dev)
        wsb = lib.query('re2e_lstm_workspace_bytes', B, H)
        ws = torch.empty(wsb // 4 + 16, device=dev)
        ybuf, cbuf = torch.zeros(T + 2, B, 2 * H, device=dev), torch.zeros(T + 2, B, 2 * H, device=dev)
        dc = torch.zeros(B, 2 * H, device=dev)
        best = [1e9, 1e9]
        for rep in range(4):
            xg = [x.clone() for x in xg0]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize()
            ev[0].record()
            lib.call('re2e_lstm_seq_fwd', xg[0].data_ptr(), xg[1].data_ptr(), whh[0].data_ptr(), whh[1].data_ptr(), ybuf.data_ptr(), cbuf.data_ptr(),
                     lens.data_ptr(), T, B, H, ws.data_ptr(), wsb)
            ev[1].record()
            lib.call('re2e_lstm_seq_bwd', xg[0].data_ptr(), xg[1].data_ptr(), whh[0].data_ptr(), whh[1].data_ptr(), dy.data_ptr(), ybuf.data_ptr(),
                     cbuf.data_ptr(), dc.data_ptr(), lens.data_ptr(), T, B, H, None, ws.data_ptr(), wsb)
            ev[2].record()
            torch.cuda.synchronize()
            if rep:
                best = [min(best[0], ev[0].elapsed_time(ev[1]) * 1e3 / T), min(best[1], ev[1].elapsed_time(ev[2]) * 1e3 / T)]
        flop = 2.0 * B * 4 * H * H * 2                   # both directions, one step
        fl = floors[(H, B)]
        out[name] = {'steps_per_layer_and_pass': T, 'fwd': {'us_per_step': round(best[0], 2), 'handoff_floor_us': fl['fwd'],
                                                            'mfma_floor_us': round(flop / (PEAK_FP32_MFMA_TFLOPS * 1e6), 2)},
                     'bwd': {'us_per_step': round(best[1], 2), 'handoff_floor_us': fl['bwd'],
                             'mfma_floor_us': round(flop / (PEAK_FP32_MFMA_TFLOPS * 1e6), 2)}}
    # the third latency-bound chain of the step: the decoder's teacher-forced loop (csrc/decloop.hip), persistent against launch-per-token
    try:
        from robust_e2e_gan_amd import ops
        B, T, L1, E, A, D, C, Fh = 32, 200, 41, 512, 320, 300, 10, 100
        g = torch.Generator().manual_seed(7)
        r = lambda *sh, scale=1.0: (torch.randn(*sh, generator=g) * scale).to(dev)
        hmask, pre = r(B, T, E).requires_grad_(True), r(B, T, A).requires_grad_(True)
        Pm = {k: torch.nn.Parameter(v) for k, v in dict(
            embed=r(50, D, scale=0.5), w_ih=r(4 * D, D + E, scale=0.08), w_hh=r(4 * D, D, scale=0.08), b_ih=r(4 * D, scale=0.1), b_hh=r(4 * D, scale=0.1),
            mlp_dec=r(A, D, scale=0.1), mlp_att=r(A, C, scale=0.5), loc_conv=r(C, 1, 1, 2 * Fh + 1, scale=0.3), gvec_w=r(1, A, scale=0.3), gvec_b=r(1, scale=0.1)).items()}
        ids = torch.randint(0, 50, (L1, B), generator=g).to(torch.int32).to(dev)
        hlens = torch.full((B,), T, dtype=torch.int32, device=dev)
        res = {}
        was = ops.DECODER_PERSIST
        for label, flag in (('launch_per_token', False), ('persistent', True)):
            ops.DECODER_PERSIST = flag
            t = []
            for bwd in (False, True):
                for rep in range(13):
                    if rep == 3:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                    if bwd:
                        z, w = ops.DecoderLoopFn.apply(hmask, pre, ids, hlens, L1, Pm)
                        z.sum().backward()
                    else:
                        with torch.no_grad():
                            z, w = ops.DecoderLoopFn.apply(hmask, pre, ids, hlens, L1, Pm)
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) / 10 * 1e3)
            res[label] = {'fwd_ms': round(t[0], 3), 'fwd_bwd_ms': round(t[1], 3), 'fwd_us_per_token': round(t[0] * 1e3 / L1, 1)}
        ops.DECODER_PERSIST = was
        res['tokens'] = L1
        res['note'] = ('ops.DecoderLoopFn alone on the chip (B=32, T\'=200, E=512: this workload\'s decoder), forward and forward+backward incl. the batched GEMMs '
                       'around the loop; per-token budgets from clock stamps: tools/dec_stamps.py')
        out['decoder_loop'] = res
    except Exception as e:                                   # (a measurement beside the metric: never fail the bench line)
        out['decoder_loop'] = {'error': repr(e)}
    out['note'] = ('us_per_step: persistent bi-LSTM kernels alone on the chip, best of 3 sequences; handoff_floor_us: the same exchange with nothing '
                   'computed (profiles/r04_handoff_probe.txt); mfma_floor_us: step FLOPs / whole-chip fp32-MFMA peak')
    return out


GRAD_TOL = 1.5e-3          # the tests' bar for a gradient tensor against the oracle's (relative to the tensor's largest entry): REPORTED here, not gated --
#                            on the bench's batch + estimated CMVN both fp32 sides sit 2-3e-3 from the float64 result (profiles/r06_grad_arbitration_fp64.txt)
PARITY_TOL = 1e-3
PARITY_KEYS = ('loss', 'loss_ctc', 'loss_att', 'enhance_loss', 'coral_loss', 'gan_loss', 'loss_D')


def _oracle_state(opt, sd, fbank_W):
    from oracle import joint as oj
    cfg = dict(enhance_layers=opt.enhance_layers, elayers=opt.elayers, mtlalpha=opt.mtlalpha, enhance_loss_lambda=opt.enhance_loss_lambda,
               coral_loss_lambda=opt.coral_loss_lambda, gan_loss_lambda=opt.gan_loss_lambda, grad_clip=opt.grad_clip, eps=opt.eps, isGAN=True,
               enhance_loss_type='L2')
    return oj.JointState(sd[0], sd[1], sd[2], fbank_W, cfg)


def cpu_baseline_and_parity(opt, sd0, fbank_W, batch, cmvn, gpu_first, sample_b=8, full_reps=3):
    """The oracle ('port') on the host cores.

    (1) parity: ONE joint step on the full batch of the GPU leg -- same synthetic batch, same initial weights (``sd0`` =
        the GPU nets' state_dicts before their first step), same cmvn -- compared with the GPU's first step.
    (2) cpu_baseline.value: the metric's own configuration (config 4, 1 warm-up + >= 3 timed): the step of (1) is the
        warm-up, ``full_reps`` more full-batch steps on identical inputs are timed, median.
    (3) ``sample_b8``: the first ``sample_b`` utterances of that batch (same T, L, V and architecture), 1 warm-up + 3 timed, next to it."""
    from oracle import joint as oj
    cores = host_cores()
    torch.set_num_threads(cores)
    log('cpu_baseline: %d threads' % cores)
    clean, mix, mix_log, targets, il, tl = batch
    B = clean.shape[0]
    t0 = time.time()
    ref = oj.joint_step(_oracle_state(opt, sd0, fbank_W), (clean, mix, mix_log, targets, il.tolist(), tl.tolist()), cmvn)
    full_s = time.time() - t0
    log('cpu oracle: full B=%d step took %.1fs' % (B, full_s))
    par = {}
    for k in PARITY_KEYS:
        a, b = gpu_first['train/' + k], float(ref[k])
        par[k] = abs(a - b) / max(abs(b), 1e-12)
    par['grad_norm'] = abs(gpu_first['grad_norm'] - ref['grad_norm_asr']) / ref['grad_norm_asr']
    eo = gpu_first['enhance_out']
    par['enhance_out_max'] = float((eo - ref['enhance_out']).abs().max() / ref['enhance_out'].abs().max())
    par = {k: float('%.3e' % v) for k, v in par.items()}
    # every gradient tensor of the three networks: max |gpu - oracle| over the tensor's largest oracle entry (the bar of tests/test_fullsize_gpu.py;
    # a tensor whose gradient is exactly zero -- att.gvec.bias in front of the softmax -- is held to an absolute floor)
    gworst = []
    for pre, key in (('enh', 'g_enh'), ('asr', 'g_asr'), ('gan', 'g_gan')):
        for k, g in gpu_first.get('grads', {}).get(pre, {}).items():
            if k in ref.get(key, {}):
                want = ref[key][k]
                err, scale = float((g - want).abs().max()), float(want.abs().max())
                gworst.append((max(err - 1e-8, 0.0) / max(scale, 1e-30), pre + '.' + k))
    gworst.sort(reverse=True)
    gmax = gworst[0][0] if gworst else None
    nz = [(e, n) for e, n in gworst if e < 1.0]          # (a ratio >= 1 is a tensor whose reference gradient is exactly zero: noise over ~0)
    grads = {'gated': False, 'tests_bar': GRAD_TOL, 'tensors': len(gworst), 'within_tests_bar': sum(1 for e, _ in nz if e <= GRAD_TOL),
             'max_rel_err': float('%.3e' % nz[0][0]) if nz else None, 'worst': [[n, float('%.3e' % e)] for e, n in nz[:3]],
             'note': 'every gradient tensor of the three networks after GPU step 1 against the fp32 oracle (max |d| / max |ref| per tensor); on this batch with '
                     'the estimated CMVN the enhancer gradients of BOTH fp32 sides are 2-3e-3 from the float64 result (profiles/r06_grad_arbitration_fp64.txt), '
                     'so this is reported and the gate stays on the scalars, the masks and the gradient norm; tests/test_fullsize_gpu.py holds every tensor to '
                     '1e-3 at this size with a fixed CMVN'}
    parity = {'tolerance': PARITY_TOL, 'rel_err': par, 'max_rel_err': max(par.values()),
              'ok': all(v <= PARITY_TOL for v in par.values()), 'gradients': grads,
              'what': 'GPU step 1 vs oracle/joint.py joint_step on the same B=%d batch, initial weights and cmvn; |a-b|/|b| for the losses and '
                      'the ASR grad norm, max|d|/max|ref| for enhance_out' % B,
              'gpu': {k: gpu_first['train/' + k] for k in PARITY_KEYS}, 'oracle': {k: float(ref[k]) for k in PARITY_KEYS}}
    del ref
    # (2) the metric's own configuration: the parity step above was the warm-up; ``full_reps`` more full-batch steps, timed, median
    L = int(tl[0])
    full_times = []
    for i in range(full_reps):
        st = _oracle_state(opt, sd0, fbank_W)            # identical inputs AND weights every repetition
        t0 = time.time()
        oj.joint_step(st, (clean, mix, mix_log, targets, il.tolist(), tl.tolist()), cmvn)
        full_times.append(time.time() - t0)
        log('cpu_baseline: full B=%d step %d took %.1fs' % (B, i + 1, full_times[-1]))
    ft = sorted(full_times)
    fmed = ft[len(ft) // 2] if ft else full_s
    # (3) a bounded sample next to it (the first ``sample_b`` utterances of that batch: same T, L, V and architecture): torch's CPU step is
    #     super-linear in the batch at this size, so the sample is the figure that is kinder to the CPU
    sb = min(sample_b, B)
    sub = (clean[:sb], mix[:sb], mix_log[:sb], targets[:sb * L], il[:sb].tolist(), tl[:sb].tolist())
    times = []
    for i in range(4):
        st = _oracle_state(opt, sd0, fbank_W)
        t0 = time.time()
        oj.joint_step(st, sub, cmvn)
        times.append(time.time() - t0)
        log('cpu_baseline: B=%d sample step %d took %.1fs%s' % (sb, i, times[-1], ' (warm-up)' if i == 0 else ''))
    timed = sorted(times[1:])
    med = timed[len(timed) // 2]
    base = {'value': round(B / fmed, 4), 'unit': 'utterances/s', 'cores': cores, 'kind': 'port',
            'sample': 'oracle/joint.py joint_step on the FULL batch of the GPU leg (B=%d, T=%d, L=%d, V=%d, config-4 architecture, same initial weights '
                      'and cmvn): 1 warm-up (the parity step) + %d timed steps, median; torch CPU fp32, %d threads'
                      % (B, clean.shape[1], L, opt.odim, len(full_times), cores),
            'seconds_timed': [round(t, 2) for t in full_times], 'seconds_warmup': round(full_s, 2),
            'sample_b8': {'utterances': sb, 'value': round(sb / med, 4), 'seconds_timed': [round(t, 2) for t in times[1:]], 'seconds_warmup': round(times[0], 2),
                          'note': 'the first %d utterances of the same batch, 1 warm-up + 3 timed steps, median' % sb}}
    return base, parity


def time_with_input(tr, batch, cmvn_d, dev, steps, world):
    """The same step fed from HOST memory (F1 / K1, data/mix_data_loader.py:264-302): the ragged per-utterance tensors of the batch
    go through data.prefetch.DevicePrefetcher every step -- pinned staging, one H2D copy per feature stream on a copy stream,
    re2e_pack_pad there, event hand-off to the step's stream -- two batches ahead of the step that consumes them.  ``value`` stays
    the resident-batch figure (the contract); this is the PCIe-inclusive one next to it."""
    from robust_e2e_gan_amd.data.prefetch import DevicePrefetcher, stage_batch
    clean, mix, mix_log, targets, il, tl = batch
    L = int(tl[0])
    samples = []
    for b, l in enumerate(il.tolist()):
        samples.append(('utt%d' % b, 'spk', clean[b, :l].contiguous(), None, mix[b, :l].contiguous(), mix_log[b, :l].contiguous(), None,
                        targets[b * L:(b + 1) * L].tolist()))
    warm = 3
    # The HOST half of the collate (ragged rows -> pinned staging buffers, ~30-50 ms per batch of CPU memcpy at this size) is the
    # DataLoader workers' job in the reference and is done once here, outside the timed loop; every timed step pays what remains on
    # the training process: one H2D copy per feature stream + re2e_pack_pad on the copy stream, two batches ahead, event hand-off.
    staged = stage_batch(samples)
    pf = DevicePrefetcher([staged] * (warm + steps), dev)      # its own copy stream, beside the step's
    it = iter(pf)
    for _ in range(warm):
        tr.step(next(it), 0.0, cmvn_d)
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for data in it:
        tr.step(data, 0.0, cmvn_d)
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    return {'ms_per_step': round(dt / steps * 1e3, 3), 'steps': steps,
            'what': 'same step, every batch uploaded from pinned HOST staging buffers by data.prefetch.DevicePrefetcher (3 x %.1f MB over PCIe on a '
                    'copy stream + re2e_pack_pad, two batches ahead, event hand-off); the ragged-row staging itself (the loader workers\' job) is '
                    'outside the timed loop' % (float(sum(il.tolist())) * 257 * 4 / 1e6)}


def spawn_ranks(n, argv):
    """``bench.py --gpus N`` (N > 1) started as ONE process: run the N ranks as fresh children under torch.distributed.run
    (this process has not touched the GPU: it only imported torch) and exit with their code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env['RE2E_BENCH_SPAWNED'] = '1'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + argv
    log('spawning %d ranks: %s' % (n, ' '.join(cmd)))
    return subprocess.call(cmd, env=env)


CONFIG_SHAPES = {2: (16, 500, 25), 3: (32, 800, 40), 4: (32, 800, 40), 5: (8, 3000, 150)}     # (B per GPU, T, L)
CONFIG_NAMES = {
    2: 'config2: asr_train.py step (clean fbank features -> VGG+3xBLSTMP-512, CTC + loc-attention decoder 300, Adadelta)',
    3: 'config3: enhance_gan_train.py step (2xBLSTM-256 mask enhancer + fbank + D basic ndf64, G-step and D-step, Adadelta)',
    4: 'config4: joint_train.py full GAN+ASR step',
    5: 'config5: joint_train.py full GAN+ASR step, long utterances',
}


def shard_batch(batch, idx, L):
    """Rows ``idx`` of a synthetic batch (strong scaling: every rank builds the SAME global batch and keeps utterances r::N)."""
    clean, mix, mix_log, targets, il, tl = batch
    ii = torch.as_tensor(idx, dtype=torch.long)
    tg = targets.view(-1, L)[ii].reshape(-1)
    return clean[ii], mix[ii], mix_log[ii], tg, il[ii], tl[ii]


def make_stepper(cfg_id, opt, nets, batch, cmvn_d, dev):
    """-> (step(), trainer, flat optimizers): one training iteration of the configuration's trainer on a batch resident in HBM."""
    from robust_e2e_gan_amd.joint_train import JointTrainer
    from robust_e2e_gan_amd import trainers
    enh, fb, asr, gan = nets
    clean, mix, mix_log, targets, il, tl = batch
    if cfg_id in (4, 5):
        tr = JointTrainer(opt, enh, fb, asr, gan)
        data = (None, None, clean.to(dev), None, mix.to(dev), mix_log.to(dev), None, targets, il, tl)
        return (lambda: tr.step(data, 0.0, cmvn_d)), tr, [tr.asr_optimizer, tr.enhance_optimizer, tr.gan_optimizer]
    if cfg_id == 3:
        tr = trainers.EnhanceGanTrainer(opt, enh, fb, gan)
        g = torch.Generator().manual_seed(4321)
        cos = torch.cos(torch.rand(clean.shape, generator=g) * 3.14159265).to(dev)          # cos of the clean/mix phase difference
        data = (None, None, clean.to(dev), None, mix.to(dev), mix_log.to(dev), cos, targets, il, tl)
        return (lambda: tr.step(data, cmvn_d)), tr, [tr.enhance_optimizer, tr.gan_optimizer]
    if cfg_id == 2:
        with torch.no_grad():                                                                 # pre-computed clean fbank features, CMVN applied
            feats = ((fb(clean.to(dev)) + cmvn_d[0]) * cmvn_d[1]).contiguous()
            for b, l in enumerate(il.tolist()):
                feats[b, l:] = 0.0
        tr = trainers.AsrTrainer(opt, asr)
        data = (None, None, feats, targets, il, tl)
        return (lambda: tr.step(data, 0.0)), tr, [tr.optimizer]
    raise SystemExit('bench: --config must be 2, 3, 4 or 5 (config 1 is the CPU plumbing case of the tests)')


DUMP_SAMPLE = 1 << 21        # elements kept of a larger output (8 MB as float32): the few outputs of a step stay under 64 MB together


def dump_outputs(path, out, tr, nets, optimizers):
    """--dump-outputs: what the last timed step computed, as ``path/<name>.npy`` -- every meter the step returned (``train/loss`` ->
    ``train_loss.npy``), the trainer's ``last`` tensors (``enhance_out``, ``enhance_feat``) and the parameters the step updated, one flat
    array per network in ``named_parameters`` order (``params_enh``, ``params_asr``, ``params_gan``).  float64 stays float64, anything
    else is written as float32.  An output of more than DUMP_SAMPLE elements is written as DUMP_SAMPLE of its flattened elements at
    sorted indices drawn from a fixed seed: the same elements for every run and build at the same shape."""
    import numpy as np
    arrays = {k.replace('/', '_'): v for k, v in out.items()}
    arrays.update(getattr(tr, 'last', {}))
    trained = {id(p) for o in optimizers for p in o.params}
    for name, m in zip(('enh', 'fbank', 'asr', 'gan'), nets):
        ps = [p.detach().reshape(-1) for p in m.parameters() if id(p) in trained] if m is not None else []
        if ps:
            arrays['params_' + name] = torch.cat(ps)
    host = {}
    for name, v in arrays.items():
        t = v.detach() if isinstance(v, torch.Tensor) else torch.tensor(float(v), dtype=torch.float64)
        t = t.to(torch.float64 if t.dtype == torch.float64 else torch.float32)
        if t.numel() > DUMP_SAMPLE:
            idx = torch.randint(0, t.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(1234)).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        host[name] = t.cpu().numpy()
    total = sum(a.nbytes for a in host.values())
    assert total <= 64 << 20, 'bench: --dump-outputs would write %d bytes' % total
    os.makedirs(path, exist_ok=True)
    for name, a in sorted(host.items()):
        np.save(os.path.join(path, name + '.npy'), a)
    log('dumped %d outputs of the last timed step (%.1f MB) to %s' % (len(host), total / 2 ** 20, path))


def time_other_config(cfg_id, dev, steps=10, warmup=3):
    """One of the other BASELINE configurations (2: asr_train, 3: enhance_gan_train, 5: joint_train on long utterances) in THIS process:
    fresh networks, its own synthetic batch and CMVN, ``warmup`` untimed + ``steps`` timed steps.  N = 1 only."""
    from robust_e2e_gan_amd.data.synthetic import make_batch
    from robust_e2e_gan_amd.joint_train import config4_opt
    opt = config4_opt()
    B, T, L = CONFIG_SHAPES[cfg_id]
    if cfg_id == 2:
        from robust_e2e_gan_amd.model.e2e_model import E2E
        from robust_e2e_gan_amd.model.feat_model import FbankModel
        torch.manual_seed(1234)
        enh, gan = None, None
        fb, asr = FbankModel(opt).to(dev).train(), E2E(opt).to(dev).train()
    else:
        enh, fb, asr, gan = build(opt, dev)
    batch = make_batch(B, T, L, opt.odim, seed=1234)
    cmvn_batches = [make_batch(B, T, L, opt.odim, seed=77 + i) for i in range(2)]
    if enh is not None:
        cmvn = synthetic_cmvn(enh, fb, cmvn_batches, dev)
    else:
        with torch.no_grad():
            f = torch.cat([fb(b[0].to(dev))[i, :l] for b in cmvn_batches for i, l in enumerate(b[4].tolist())], 0)
            cmvn = torch.stack([-f.mean(0), 1.0 / f.std(0)]).cpu()
    step, tr, _ = make_stepper(cfg_id, opt, (enh, fb, asr, gan), batch, cmvn.to(dev), dev)
    host_ms = None
    for _ in range(warmup):
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        step()
        host_ms = (time.perf_counter() - h0) * 1e3       # enqueue time of ONE step issued into an idle GPU (no back-pressure)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    utt_s = B * steps / dt
    out = {'ms': round(dt / steps * 1e3, 3), 'utt_s': round(utt_s, 2), 'frac': round(utt_s * FLOP_PER_UTT[cfg_id] / (PEAK_FP32_MFMA_TFLOPS * 1e12), 4),
           'steps': steps, 'warmup': warmup, 'workload': '%s, B=%d, T=%d, L=%d' % (CONFIG_NAMES[cfg_id], B, T, L),
           'host_enqueue_ms': round(host_ms, 2) if host_ms is not None else None,
           'host_bound': bool(host_ms is not None and dt / steps * 1e3 < 1.3 * host_ms)}
    del step, tr, enh, fb, asr, gan
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--config', type=int, default=4, choices=(2, 3, 4, 5), help='BASELINE.json configuration (default 4 = the metric)')
    ap.add_argument('--scaling', default='weak', choices=('weak', 'strong'),
                    help='weak: the configuration\'s batch per GPU; strong: that batch is the GLOBAL batch, rank r keeps utterances r::N')
    ap.add_argument('--batch', type=int, default=None)
    ap.add_argument('--frames', type=int, default=None)
    ap.add_argument('--labels', type=int, default=None)
    ap.add_argument('--full', action='store_true',
                    help='also run every measurement and check beside the headline: extra untimed steps, input_side, rooflines, other '
                         'configurations, cpu_baseline and parity (the --no-* options below drop parts of it)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-roofline', action='store_true')
    ap.add_argument('--no-input-side', action='store_true', help='skip the second timed loop that feeds HOST batches through the device prefetcher')
    ap.add_argument('--no-other-configs', action='store_true', help='skip the 5-step runs of configurations 2, 3 and 5 (N = 1, --config 4 only)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step computed (rank 0) as DIR/<name>.npy, see dump_outputs()')
    a = ap.parse_args()
    if a.steps < 1:
        ap.error('--steps must be at least 1')

    if a.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(spawn_ranks(a.gpus, sys.argv[1:]))

    from robust_e2e_gan_amd import dist as rdist
    from robust_e2e_gan_amd import lib
    from robust_e2e_gan_amd.data.synthetic import make_batch
    from robust_e2e_gan_amd.joint_train import JointTrainer, config4_opt
    rank, world, local = rdist.init_from_env()
    assert world == a.gpus, '--gpus %d but WORLD_SIZE=%d' % (a.gpus, world)
    assert torch.cuda.is_available(), 'bench.py needs a GPU (no CPU fallback)'
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    assert lib.query('re2e_device_ok') == 1, 'not a gfx950 device'

    opt = config4_opt()
    log('building networks')
    if a.config == 2:
        from robust_e2e_gan_amd.model.e2e_model import E2E
        from robust_e2e_gan_amd.model.feat_model import FbankModel
        torch.manual_seed(1234)
        enh, gan = None, None
        fb, asr = FbankModel(opt).to(dev).train(), E2E(opt).to(dev).train()
    else:
        enh, fb, asr, gan = build(opt, dev)
    cB, cT, cL = CONFIG_SHAPES[a.config]
    B, T, L = a.batch or cB, a.frames or cT, a.labels or cL
    if a.scaling == 'strong':
        if B < world:
            raise SystemExit('bench: strong scaling needs at least one utterance per rank (global batch %d, %d ranks)' % (B, world))
        gbatch = make_batch(B, T, L, opt.odim, seed=1234)                       # the SAME global batch on every rank
        # ONE batch over the ranks: the discriminator's BatchNorm statistics are those of the global batch (synchronised BatchNorm:
        # three small all-reduces per layer and pass) when the shards are equal; ragged shards keep per-rank statistics
        opt.sync_bn = world > 1 and B % world == 0 and a.config in (4, 5)      # (JointTrainer implements it; config 3's trainer keeps per-rank statistics)
        batch = shard_batch(gbatch, rdist.shard_indices(B, rank, world), L)
        global_b = B
    else:
        batch = make_batch(B, T, L, opt.odim, seed=1234 + rank)
        global_b = B * world
    local_b = int(batch[0].shape[0])
    log('synthetic batch ready (%d utterances on this rank); computing cmvn' % local_b)
    cmvn_batches = [make_batch(cB if a.batch is None else B, T, L, opt.odim, seed=77 + i) for i in range(2)]
    if enh is not None:
        cmvn = synthetic_cmvn(enh, fb, cmvn_batches, dev)
    else:                                            # config 2: CMVN of the clean features themselves
        with torch.no_grad():
            f = torch.cat([fb(b[0].to(dev))[i, :l] for b in cmvn_batches for i, l in enumerate(b[4].tolist())], 0)
            cmvn = torch.stack([-f.mean(0), 1.0 / f.std(0)]).cpu()
    cmvn_d = cmvn.to(dev)
    step, tr, optimizers = make_stepper(a.config, opt, (enh, fb, asr, gan), batch, cmvn_d, dev)
    joint = a.config in (4, 5)
    parity_run = world == 1 and joint and not a.no_cpu_baseline     # runs in which --full has a parity gate
    want_cpu = a.full and parity_run
    sd0 = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in (enh, asr, gan)] if want_cpu else None

    log('warm-up (%d steps)' % a.warmup)
    gpu_first, host_ms = None, None
    # the parity gate needs the first step un-timed; a plain run warms up the same way, so both time the same steps
    nwarm = max(a.warmup, 1 if parity_run else 0)
    for i in range(nwarm):
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        out = step()
        host_ms = (time.perf_counter() - h0) * 1e3       # enqueue time of ONE step issued into an idle GPU (no back-pressure)
        torch.cuda.synchronize()
        if i == 0 and want_cpu:                          # the step the parity gate compares: first update from the initial weights
            gpu_first = JointTrainer.to_floats(out)
            gpu_first['enhance_out'] = tr.last['enhance_out'].detach().cpu()
            # ... and every gradient tensor of the three networks (the kernels leave them unclipped in p.grad: the clip coefficient is applied
            # inside the fused optimizer step)
            gpu_first['grads'] = {pre: {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}
                                  for pre, m in (('enh', enh), ('asr', asr), ('gan', gan))}
        log('warm-up step %d done (host enqueue %.1f ms)' % (i, host_ms))
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = step()
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    dt = time.perf_counter() - t0
    if a.dump_outputs and rank == 0:                 # before the untimed steps below move the weights on
        dump_outputs(a.dump_outputs, out, tr, (enh, fb, asr, gan), optimizers)
    comm = None
    if world > 1 and a.full:
        # ONE more, untimed step with an event timeline of its gradient all-reduces: when each was issued and when the step could
        # continue behind it, in ms from the step's start, on every rank -- the first multi-GPU run shows exposed communication directly
        rdist.COMM_TIMING = True
        ev0 = torch.cuda.Event(enable_timing=True)
        ev0.record()
        step()
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record()
        torch.cuda.synchronize()
        rdist.COMM_TIMING = False
        mine = {'rank': rank, 'step_ms': round(ev0.elapsed_time(ev1), 3),
                'allreduces': [{'bytes': b, 'issued_ms': i, 'done_ms': d} for b, i, d in rdist.comm_report(ev0)]}
        every = [None] * world
        torch.distributed.all_gather_object(every, mine)
        comm = every
    rank_ms = [dt / a.steps * 1e3]
    if world > 1:
        mine = torch.tensor([dt], device=dev)
        every = [torch.zeros_like(mine) for _ in range(world)]
        torch.distributed.all_gather(every, mine)
        rank_ms = [float(t.item()) / a.steps * 1e3 for t in every]
        dt = max(float(t.item()) for t in every)            # MAX over ranks
    log('timed region done: %.3fs for %d steps' % (dt, a.steps))
    losses = JointTrainer.to_floats(out)
    aborts = lib.query('re2e_lstm_abort_count')
    if world > 1:                                            # every rank fails together (a lone SystemExit would hang the others' collectives)
        flag = torch.tensor([float(aborts)], device=dev)
        torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MAX)
        aborts = int(flag.item())
    if aborts != 0:        # a persistent recurrence gave up on a peer workgroup: its outputs are NaN, the numbers mean nothing
        raise SystemExit('bench: %d recurrent sequences were aborted by a persistent kernel (rank %d)' % (aborts, rank))
    if not all(v == v and abs(v) != float('inf') for v in losses.values()):
        raise SystemExit('bench: non-finite losses after the timed region: %r' % (losses,))
    # ONE more, untimed step under the host-side FLOP meter (robust_e2e_gan_amd/flops.py): the matrix-core FLOPs the launches of a step really
    # execute -- valid rows of the ragged batch, row-limited Winograd heights, Winograd-reduced products -- and their direct-form equivalent
    fmeter = None
    if a.full:
        from robust_e2e_gan_amd import flops as rflops
        with rflops.meter() as fmeter:
            step()
        torch.cuda.synchronize()
        exe_flop, direct_flop = rflops.totals(fmeter)
    replicas_identical = None
    rccl_ranks = torch.distributed.get_world_size() if (world > 1 and torch.distributed.is_initialized()) else 1
    if world > 1:
        # replicas must still be identical after the timed steps: the all-reduced gradients and the shared NaN gate give
        # every rank the same update (D's BatchNorm running statistics are per replica and not part of this check)
        chk = torch.stack([o.flat.double().sum() for o in optimizers])
        lo, hi = chk.clone(), chk.clone()
        torch.distributed.all_reduce(lo, op=torch.distributed.ReduceOp.MIN)
        torch.distributed.all_reduce(hi, op=torch.distributed.ReduceOp.MAX)
        replicas_identical = bool(torch.equal(lo, hi))
        if not replicas_identical:
            raise SystemExit('bench: replicas differ after %d data-parallel steps: %r vs %r' % (a.steps, lo.tolist(), hi.tolist()))
    input_side = None
    if a.full and joint and not a.no_input_side:
        input_side = time_with_input(tr, batch, cmvn_d, dev, a.steps, world)
    if rank != 0:
        return
    value = global_b * a.steps / dt
    default_shape = (B, T, L) == CONFIG_SHAPES[a.config]
    metric = 'joint_train utterances/sec' if joint else {2: 'asr_train utterances/sec', 3: 'enhance_gan_train utterances/sec'}[a.config]
    line = {
        'metric': metric, 'value': round(value, 3), 'unit': 'utterances/s', 'n_gpus': world, 'steps': a.steps,
        'warmup': nwarm, 'ms_per_step': round(dt / a.steps * 1e3, 3), 'higher_is_better': True, 'scaling': a.scaling, 'vs_baseline': None,
        'dtype': 'f32', 'data': 'synthetic',
        'config': {'workload': '%s, B=%d %s, T=%d, F=257->80, L=%d, V=4233%s' % (
                       CONFIG_NAMES[a.config], B, 'per GPU' if a.scaling == 'weak' else 'GLOBAL (rank r keeps utterances r::N)', T, L,
                       ', enhancer 2xBLSTM-256, VGG+3xBLSTMP-512, loc-attention decoder 300, D basic ndf64, Adadelta' if joint else ''),
                   'global_batch': global_b, 'per_rank_batch': local_b, 'parallelism': 'dp%d' % world, 'coral_loss_lambda': opt.coral_loss_lambda,
                   # the synthetic batch is ragged like a collated one (data/synthetic.py: lengths T .. 0.7 T, sorted): the reference packs its
                   # sequences and cuts its VGG output, and so do the products around the recurrences and the VGG stack here
                   'utterance_lengths': '%d..%d frames (mean %.0f of T=%d)' % (int(batch[4].min()), int(batch[4].max()), float(batch[4].float().mean()), T)},
        # whole-step fraction of the fp32-MFMA roofline: utterances/s x SURVEY 8(d) FLOP per utterance / (N x 157.3 TFLOP/s); the FLOP
        # count holds for the configuration's own (T, L) whatever the batch, so it is given for weak and strong scaling alike
        'step_mfma_frac': round(value * FLOP_PER_UTT[a.config] / (world * PEAK_FP32_MFMA_TFLOPS * 1e12), 4) if (T, L) == CONFIG_SHAPES[a.config][1:] else None,
    }
    if fmeter is not None:
        line.update({
            # ... and the honest twin of it (round 6): the FLOP count above prices every padded row of the (B, Tmax) box, while the step no longer
            # computes them (products over the valid rows, row-limited VGG launches).  step_executed_* = matrix-core FLOPs of the launches one step
            # of THIS rank really made (host-side meter over lib.call, robust_e2e_gan_amd/flops.py: valid rows, row-limited heights, Winograd-reduced
            # products) over the measured step time; flop_per_utt_valid_rows = the direct-form equivalent of those launches per utterance (what
            # SURVEY 8(d)'s figure becomes when padding is not counted); step_valid_rows_frac = utt/s x that / peak
            'step_executed_tflop': round(exe_flop / 1e12, 4),
            'step_executed_tflops': round(exe_flop / (dt / a.steps) / 1e12, 2),
            'step_executed_frac': round(exe_flop / (dt / a.steps) / (PEAK_FP32_MFMA_TFLOPS * 1e12), 4),
            'flop_per_utt_valid_rows': round(direct_flop / max(local_b, 1) / 1e9, 2),
            'flop_per_utt_valid_rows_unit': 'GFLOP (direct form, padded rows not counted; SURVEY 8(d) with padding: %.2f)' % (FLOP_PER_UTT[a.config] / 1e9),
            'step_valid_rows_frac': round(direct_flop / (dt / a.steps) / (PEAK_FP32_MFMA_TFLOPS * 1e12), 4),
            'step_executed_by_entry_point_gflop': {k: round(v / 1e9, 1) for k, v in sorted(fmeter.items(), key=lambda kv: -kv[1]) if k != rflops.DIRECT},
        })
    line.update({
        'default_shape': default_shape,
        'final_losses': {k: round(v, 5) for k, v in losses.items()}, 'persistent_kernel_aborts': aborts,
        'rccl_ranks': rccl_ranks, 'replicas_identical': replicas_identical, 'self_spawned': os.environ.get('RE2E_BENCH_SPAWNED') == '1',
        'rank_ms_per_step': {'min': round(min(rank_ms), 3), 'max': round(max(rank_ms), 3)},
        'host_enqueue_ms_per_step': round(host_ms, 2) if host_ms is not None else None,
        'full': a.full,
    })
    if comm is not None:
        line['comm_timeline'] = {'what': 'one extra untimed step per rank: every gradient all-reduce with the time it was issued and the time the step '
                                         'could continue behind it (HIP events, ms from the step\'s start); ASR (largest) is issued after backward '
                                         'phase 1 and runs under the enhancer\'s backward, the enhancer\'s and D\'s follow at the end', 'ranks': comm}
    if input_side is not None:
        input_side['delta_ms'] = round(input_side['ms_per_step'] - line['ms_per_step'], 3)
        line['input_side'] = input_side
    if a.full and not a.no_roofline:
        line['roofline'] = conv_roofline(dev)
        line['roofline_engine'] = engine_roofline(dev)
        line['roofline_chain'] = chain_roofline(dev)
    if a.full and world == 1 and a.config == 4 and default_shape and not a.no_other_configs:
        # step_mfma_frac of the other configurations, measured by THIS run (5 timed steps each): `frac` = utt/s x SURVEY 8(d) FLOP / fp32-MFMA peak
        line['other_configs'] = {str(c): time_other_config(c, dev) for c in (2, 3, 5)}
        log('other configurations: %s' % {c: v['ms'] for c, v in line['other_configs'].items()})
    if want_cpu:
        from robust_e2e_gan_amd.model.feat_model import mel_matrix
        line['cpu_baseline'], line['parity'] = cpu_baseline_and_parity(opt, sd0, torch.from_numpy(mel_matrix()), batch, cmvn, gpu_first)
        print(json.dumps(line))
        if not line['parity']['ok']:
            raise SystemExit('bench: parity gate FAILED (tolerance %g): %r' % (PARITY_TOL, line['parity']['rel_err']))
        return
    print(json.dumps(line))


if __name__ == '__main__':
    main()
