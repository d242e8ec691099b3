"""CPU-only: the C-ABI library loads, exports every symbol include/re2e.h declares, and the ctypes
signature table agrees with the header's argument TYPES.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ctype_of(decl):
    """C parameter (or return) declaration -> the ctypes class that must stand for it."""
    d = re.sub(r'\bconst\b', '', decl).strip()
    if '*' in d:                      # every pointer parameter is passed as an address (device pointers, host length arrays)
        return ctypes.c_void_p
    base = re.sub(r'\s+\w+$', '', d).strip() if re.search(r'\s\w+$', d) else d          # drop the parameter name
    table = {'int': ctypes.c_int, 'long': ctypes.c_long, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t,
             're2e_stream_t': ctypes.c_void_p, 'unsigned': ctypes.c_uint, 'double': ctypes.c_double,
             'unsigned long long': ctypes.c_ulonglong}
    assert base in table, 'include/re2e.h: unhandled parameter type %r' % decl
    return table[base]


def _header_decls():
    """name -> (restype, [argtypes...]) parsed from include/re2e.h."""
    src = open(os.path.join(ROOT, 'include', 're2e.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    decls = {}
    for m in re.finditer(r'([\w\s\*]+?)\b(re2e_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if ret.startswith('typedef') or not ret:
            continue
        ret = ret.split('\n')[-1].strip()
        params = [] if args in ('', 'void') else [a.strip() for a in args.split(',')]
        res = ctypes.c_char_p if ret.replace(' ', '') == 'constchar*' else _ctype_of(ret + ' r')
        decls[name] = (res, [_ctype_of(a) for a in params])
    return decls


def test_library_exports_every_declared_symbol():
    from robust_e2e_gan_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    so = ctypes.CDLL(lib.LIB_PATH)
    decls = _header_decls()
    assert len(decls) >= 50
    for name in decls:
        assert hasattr(so, name), 'symbol %s declared in include/re2e.h is not exported' % name
    abi_macro = int(re.search(r'#define\s+RE2E_ABI_VERSION\s+(\d+)', open(os.path.join(ROOT, 'include', 're2e.h')).read()).group(1))
    assert so.re2e_version() == abi_macro == lib.ABI_VERSION, 'library, header and ctypes table must carry the same ABI version'


def test_ctypes_table_matches_header():
    """Argument by argument: the ctypes class in lib.SIGNATURES must be the one the header's C type maps to (pointer ->
    c_void_p, int -> c_int, long -> c_long, float -> c_float, size_t -> c_size_t), and so must the return type -- with
    up to 27 positional arguments a swapped int/long or float/int pair would otherwise corrupt a call silently.  The
    last header parameter of every launching entry point is ``re2e_stream_t stream``; lib.SIGNATURES lists it too."""
    from robust_e2e_gan_amd import lib
    decls = _header_decls()
    assert set(decls) == set(lib.SIGNATURES), set(decls) ^ set(lib.SIGNATURES)
    for name, (res, args) in decls.items():
        tres, targs = lib.SIGNATURES[name]
        assert tres is res, (name, 'return', tres, res)
        assert len(targs) == len(args), (name, len(args), len(targs))
        for i, (a, b) in enumerate(zip(targs, args)):
            assert a is b, '%s: argument %d is %s in lib.SIGNATURES but %s in include/re2e.h' % (name, i, a.__name__, b.__name__)


_LSTM_SWITCHES = ('RE2E_LSTM_PERSIST', 'RE2E_LSTM_PERSIST_BWD', 'RE2E_LSTM_FWD2', 'RE2E_LSTM_BWD3', 'RE2E_LSTM_BWD_UW')
# (T, B, H, environment, family, parameters, grid, dynamic LDS bytes) on a 256-CU chip; None: not pinned
_FWD_PLANS = [
    (60, 32, 256, {}, 'fwd_persist', dict(waves=8, qn=4), '32x1x2', 163840),
    (60, 40, 320, {}, 'fwd_persist', dict(waves=8, qn=5), '40x2x2', 33808),
    (60, 70, 256, {}, 'fwd_persist', dict(waves=8, qn=4), '32x3x2', 33808),
    (60, 40, 64, {}, 'fwd_persist', dict(waves=4, qn=2), '8x2x2', 163840),
    (60, 3, 32, {}, 'fwd_persist', dict(waves=4, qn=1), '4x1x2', 163840),
    (60, 64, 512, {}, 'fwd2_persist', dict(tiles=4, nj=8), '32x4x2', 32784),
    (60, 24, 512, {}, 'fwd2_persist', dict(tiles=4, nj=8), '32x2x2', 163840),
    (60, 16, 512, {}, 'fwd2_persist', dict(tiles=2, nj=8), '64x1x2', 163840),
    (60, 8, 256, {}, 'fwd2_persist', dict(tiles=1, nj=4), '64x1x2', 163840),
    (60, 12, 128, {}, 'fwd2_persist', dict(tiles=1, nj=2), '32x1x2', 163840),
    (60, 9, 320, {}, 'fwd2_persist', dict(tiles=2, nj=5), '40x1x2', 163840),
    (60, 128, 512, {}, 'fwd2_step', dict(tiles=4, nj=8), '32x8x2', 32784),
    (60, 32, 384, {}, 'fwd_step', dict(waves=8), '48x1x2', 33792),
    (60, 160, 256, {}, 'fwd_step', dict(waves=8), None, None),
    (1, 8, 256, {}, 'fwd2_step', dict(tiles=1), None, None),
    (1, 32, 256, {}, 'fwd_step', dict(waves=8), None, None),
    (60, 64, 512, {'RE2E_LSTM_FWD2': '0'}, 'fwd_persist', dict(waves=8, qn=8), '64x2x2', 33808),
    (60, 32, 256, {'RE2E_LSTM_PERSIST': '0'}, 'fwd_step', dict(waves=8), None, None),
]
_BWD_PLANS = [
    (60, 32, 256, {}, 'bwd3', dict(un=16, tpw=4), '16x2x2', 147456),
    (60, 40, 320, {}, 'bwd3', dict(un=16, tpw=5), '20x3x2', 147456),
    (60, 8, 256, {}, 'bwd3', dict(un=8, tpw=4), '32x1x2', 147456),
    (60, 64, 512, {}, 'bwd3', dict(un=16, tpw=8), '32x4x2', 0),
    (60, 3, 32, {}, 'bwd_persist', dict(tpw=1, uw=1), '4x1x2', 147456),
    (60, 128, 512, {}, 'bwd_persist', dict(tpw=4, uw=2), '32x4x2', 0),
    (60, 256, 512, {}, 'bwd_step', dict(jt=2), None, None),
    (1, 32, 256, {}, 'bwd_step', dict(jt=2), None, None),
    (1, 3, 32, {}, 'bwd_step', dict(jt=1), None, None),
    (60, 32, 256, {'RE2E_LSTM_BWD3': '0'}, 'bwd_persist', dict(tpw=2, uw=1), '32x1x2', 147456),
    (60, 40, 320, {'RE2E_LSTM_BWD3': '0', 'RE2E_LSTM_BWD_UW': '2'}, 'bwd_persist', dict(tpw=3, uw=2), '20x2x2', None),
    (60, 32, 256, {'RE2E_LSTM_PERSIST_BWD': '0'}, 'bwd_step', {}, None, None),
]
# what csrc/lstm.hip instantiates per family: (first, second) parameter.  A copy of its RE2E_*_ALL tables (the library's own is_built checks
# every plan against those): it has to follow them when an instantiation is added or dropped.
_LSTM_BUILT = {
    'fwd2_persist': ('tiles', 'nj', {(t, n) for t in (1, 2, 4) for n in (1, 2, 4, 5, 8)}),
    'fwd2_step': ('tiles', 'nj', {(t, n) for t in (1, 2, 4) for n in (1, 2, 4, 5, 8)}),
    'fwd_persist': ('waves', 'qn', {(8, 8), (8, 5), (8, 4), (8, 3), (4, 4), (4, 2), (4, 1)}),
    'fwd_step': ('waves', None, {(w, None) for w in (1, 2, 4, 8, 16)}),
    'bwd3': ('un', 'tpw', {(u, t) for u in (8, 16) for t in range(1, 9)}),
    'bwd_persist': ('tpw', 'uw', {(t, u) for t in (1, 2, 3, 4) for u in (1, 2)}),
    'bwd_step': ('jt', None, {(1, None), (2, None)}),
}


def test_lstm_plan_table(monkeypatch):
    """re2e_lstm_plan (the host functions re2e_lstm_seq_fwd / _bwd choose their kernel with) on a 256-CU chip: the kernel family, its
    parameters, grid and dynamic LDS per shape and switch; then over a sweep of shapes and two chip sizes every persistent plan keeps its
    whole grid resident and every plan names an instantiation that is built.  No device is touched (cus > 0)."""
    from robust_e2e_gan_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    for backward, table in ((False, _FWD_PLANS), (True, _BWD_PLANS)):
        for T, B, H, env, family, params, grid, lds in table:
            for k in _LSTM_SWITCHES:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got = lib.lstm_plan(T, B, H, backward=backward, cus=256)
            where = (T, B, H, env, got)
            assert got['family'] == family, where
            for k, v in params.items():
                assert int(got[k]) == v, where
            assert grid is None or got['grid'] == grid, where
            assert lds is None or int(got['lds']) == lds, where
    for k in _LSTM_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for cus in (64, 256):
        for B in (1, 8, 16, 17, 32, 64, 128, 300):
            for H in (8, 32, 64, 128, 256, 320, 384, 512, 1024):
                for backward in (False, True):
                    got = lib.lstm_plan(60, B, H, backward=backward, cus=cus)
                    where = (cus, B, H, got)
                    ka, kb, built = _LSTM_BUILT[got['family']]
                    assert (int(got[ka]), int(got[kb]) if kb else None) in built, where
                    gx, gy, gz = (int(v) for v in got['grid'].split('x'))
                    assert gz == 2 and int(got['lds']) >= 0, where
                    if got['family'] in ('fwd2_persist', 'fwd_persist', 'bwd3', 'bwd_persist'):
                        assert gx * gy * gz <= cus, where
    with pytest.raises(lib.Re2eError):          # no kernel for this width: an error code, not a plan
        lib.lstm_plan(60, 8, 12, cus=256)


_NT, _NN, _TN = (0, 1), (0, 0), (1, 0)
_NONE, _TANH, _RELU, _MASK = 0, 1, 2, 5          # RE2E_ACT_*
# (form, M, N, K, activation, row map, filler stream) -> the plan on a 256-CU chip, all operands 16-byte aligned with natural leading
# dimensions.  Dumped from the commit BEFORE plan_gemm existed, by a reader over its try-and-fall-through functions: a row that changes is a
# change of behaviour.  need: workspace bytes the route uses; ws: what re2e_gemm_workspace_bytes answers (either stream role, the pipeline's
# run-time fallback included).
_GEMM_PLANS = [
    (_NT, 5, 3, 7, _NONE, 0, 0, dict(route='engine', tile='128x128x16', vec=0, splits=1, m1=5, need=0, ws=0)),
    (_NT, 17, 33, 72, _NONE, 0, 0, dict(route='skinny_wg', vec=1, ws=0)),
    (_NT, 32, 20, 66, _NONE, 0, 0, dict(route='skinny_wg', vec=0, ws=0)),
    (_NT, 8, 130, 512, _TANH, 0, 0, dict(route='engine', tile='32x128x32', vec=1, splits=8, m1=8, need=33280, ws=524288)),
    (_NT, 8, 36, 8196, _NONE, 0, 0, dict(route='engine', tile='32x128x32', vec=1, splits=64, m1=8, need=73728, ws=4194304)),
    (_NT, 4352, 2046, 16, _NONE, 0, 0, dict(route='engine', tile='256x128x16', vec=1, splits=1, m1=4096, need=0, ws=0)),      # + 64x64 tail
    (_NT, 4352, 2046, 16, _NONE, 0, 1, dict(route='engine', tile='128x128x16', vec=1, splits=1, m1=4352, need=0, ws=0)),
    (_NT, 12288, 2048, 64, _NONE, 0, 0, dict(route='pipeline', variant=3, tile='256x128x16', n_dp=768, g_sk=0, need=0, ws=0)),
    (_NT, 12288, 2048, 64, _NONE, 0, 1, dict(route='pipeline', variant=6, tile='128x128x16', n_dp=1536, g_sk=0, need=0, ws=0)),
    (_NT, 12800, 512, 260, _NONE, 0, 0, dict(route='pipeline', variant=3, tile='256x128x16', n_dp=200, g_sk=0, need=0, ws=33554432)),
    (_NT, 6400, 512, 4240, _NONE, 0, 0, dict(route='pipeline', variant=8, tile='128x64x16', n_dp=256, g_sk=256, need=16777216, ws=65536000)),
    (_NT, 6400, 512, 4240, _NONE, 1, 0, dict(route='pipeline', variant=8, tile='128x64x16', n_dp=256, g_sk=256, need=16777216, ws=65536000)),
    (_NT, 300, 516, 200, _NONE, 0, 0, dict(route='pipeline', variant=8, tile='128x64x16', n_dp=27, g_sk=0, need=0, ws=0)),
    (_NT, 255, 516, 200, _NONE, 0, 0, dict(route='engine', tile='128x128x16', vec=1, splits=1, m1=255, need=0, ws=0)),
    (_NT, 12800, 260, 512, _MASK, 0, 0, dict(route='engine', tile='256x128x16', vec=1, splits=1, m1=12800, need=0, ws=0)),
    (_NN, 130, 64, 257, _RELU, 0, 0, dict(route='engine', tile='128x128x16', vec=0, splits=1, m1=130, need=0, ws=0)),
    (_NN, 32, 512, 1200, _NONE, 0, 0, dict(route='skinny_wg', vec=1, ws=1245184)),
    (_TN, 1200, 812, 1312, _NONE, 0, 0, dict(route='engine', tile='128x128x16', vec=1, splits=5, m1=1200, need=19488000, ws=19488000)),
    (_TN, 2048, 512, 12800, _NONE, 0, 0, dict(route='engine', tile='256x128x16', vec=1, splits=8, m1=2048, need=33554432, ws=33554432)),
    (_TN, 2048, 512, 12800, _NONE, 0, 1, dict(route='engine', tile='128x128x16', vec=1, splits=8, m1=2048, need=33554432, ws=33554432)),
    (_TN, 8, 4, 40000, _NONE, 0, 0, dict(route='engine', tile='128x128x16', vec=1, splits=156, m1=8, need=19968, ws=19968)),
]
# what the dense entry points instantiate.  A copy of csrc/igemm.hip's tile table as run_engine's BUILT masks admit it per form and VEC, and of
# csrc/gemm_nt.hip's variant table: it has to follow them when an instantiation is added or dropped.
_ENGINE_BUILT = {
    (_NT, 1): {'128x128x16', '256x128x16', '32x128x32'}, (_NT, 0): {'128x128x16', '32x128x32'},
    (_NN, 1): {'128x128x16', '32x128x32'}, (_NN, 0): {'128x128x16', '32x128x32'},
    (_TN, 1): {'128x128x16', '256x128x16'}, (_TN, 0): {'128x128x16'},
}
_PIPELINE_BUILT = {3: '256x128x16', 6: '128x128x16', 8: '128x64x16'}


def test_gemm_plan_table():
    """re2e_gemm_plan (csrc/igemm.hip plan_gemm, which re2e_gemm, re2e_gemm_nt_rows, re2e_gemm_tn_rows and the K-sliced batches choose
    their kernel with) on a 256-CU chip against the table above; then over a sweep of shapes, forms, stream roles and two chip sizes every
    plan names something that is built, its workspace does not depend on the stream role, and a stream-K tail has at least two workgroups.
    No device is touched where cus > 0."""
    from robust_e2e_gan_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    for form, M, N, K, act, rowmap, filler, want in _GEMM_PLANS:
        got = lib.gemm_plan(form[0], form[1], M, N, K, act=act, rowmap=bool(rowmap), filler=bool(filler), cus=256)
        where = (form, M, N, K, act, rowmap, filler, got)
        for k, v in want.items():
            assert got[k] == str(v), (k, where)
    so = lib.load()
    for cus in (64, 256, 0):          # 0: the chip re2e_gemm_workspace_bytes itself plans for (256 CUs without a device)
        for form in (_NT, _NN, _TN):
            for M in (1, 31, 32, 33, 255, 256, 2047, 2048, 12800):
                for N in (4, 64, 130, 2046, 2048):
                    for K in (16, 63, 64, 128, 8192, 8196):
                        plans = [lib.gemm_plan(form[0], form[1], M, N, K, filler=f, cus=cus) for f in (False, True)]
                        for got, other in (plans, plans[::-1]):
                            where = (cus, form, M, N, K, got)
                            if got['route'] == 'engine':
                                assert got['tile'] in _ENGINE_BUILT[form, int(got['vec'])], where
                                assert int(got['splits']) >= 1 and int(got['vec']) in (0, 1), where
                                m1 = int(got['m1'])
                                assert m1 == M or (form == _NT and got['vec'] == '1' and got['tile'] == '256x128x16' and 2048 <= m1 < M), where
                            elif got['route'] == 'pipeline':
                                assert _PIPELINE_BUILT.get(int(got['variant'])) == got['tile'], where
                                n_dp, g_sk = int(got['n_dp']), int(got['g_sk'])
                                assert n_dp + g_sk >= 1 and (g_sk == 0 or g_sk >= 2), where
                            else:
                                assert got['route'] == 'skinny_wg' and M <= 32 and form != _TN, where
                            assert int(got['ws']) >= int(got['need']), where
                            assert int(got['ws']) >= int(other['ws']), where          # i.e. equal: the workspace is sized without a stream
                            if cus == 0:
                                assert int(got['ws']) == so.re2e_gemm_workspace_bytes(form[0], form[1], M, N, K), where


# what the convolution entry points instantiate.  A copy of the BUILT masks of csrc/igemm.hip's conv_engine / re2e_conv_wgrad, of thinconv.hip's
# launch_cout1 / conv_cin1_fwd_kernel instantiations and of conv3x3.hip's HALO_GO: it has to follow them when an instantiation is added or dropped.
_CONV_ENGINE_BUILT = {
    ('engine', 1): {'128x128x16', '256x128x16', '256x64x16', '256x32x32'}, ('engine', 0): {'128x128x16', '256x64x16', '256x32x32'},
    ('wgrad_engine', 1): {'128x128x16', '256x64x16', '256x32x32', '192x64x16'}, ('wgrad_engine', 0): {'128x128x16', '256x64x16', '256x32x32'},
}
_COUT1_BUILT = {(16, 3, 3, 1), (16, 2, 2, 1), (64, 4, 4, 2)} | {(L, 0, 0, 0) for L in (1, 2, 4, 8, 16, 32, 64)}


def _check_conv_plan_is_built(got, where):
    route = got.get('route')
    if got['family'] != 'direct':
        assert got['family'] in ('wino3x3', 'wino4x4') and int(got['ws']) > 0, where
    elif route in ('engine', 'wgrad_engine'):
        assert got['tile'] in _CONV_ENGINE_BUILT[route, int(got['vec'])], where
    elif route == 'pipeline':
        assert _PIPELINE_BUILT.get(int(got['variant'])) == got['tile'] and int(got['n_dp']) >= 1, where
    elif route == 'cout1':
        assert tuple(int(got[k]) for k in ('L', 'kh', 'kw', 'ch')) in _COUT1_BUILT and int(got['grid']) >= 1, where
    elif route == 'cin1_fwd':
        assert got['taps'] in ('3x3', '4x4') and int(got['grid']) >= 1, where
    elif route == 'halo':
        assert got['patch'] in ('16x16', '32x8') and got['dir'] in ('1', '-1') and got['relu'] in ('0', '1') and got['grid'] == got['items'], where
    else:
        assert route in ('cout1_rows', 'wgrad_cin1', 'wgrad_cout1'), where


def test_conv_plan_table():
    """re2e_conv_plan (csrc/igemm.hip plan_conv_layer / plan_conv, which ops.py and the convolution entry points choose their kernels with) on a
    256-CU chip against tests/golden/conv_plan_table.json: rows of [direction, N, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW, activation,
    RE2E_CONV_* flags] -> the plan.  The table was dumped from the commit BEFORE plan_conv existed, by a reader over its choosers -- ops.py's
    predicates as Conv2dFn / conv_dgrad combined them, and its entry points with every launch site recording instead of enqueueing: a row
    that changes is a change of behaviour.  It holds every convolution pass of one bench.py step, every CONVS row of test_kernels_gpu.py and
    the boundaries between the routes, each also with unaligned operands, behind RE2E_NO_WINOGRAD and on a filler stream where that changes
    the plan.  Then over a sweep of sizes, directions, stream roles and two chip sizes every plan names something that is built, the weight
    gradient's workspace covers its need and does not depend on the stream role, and no Winograd launch gets a tensor of 2 GiB or more.  No
    device is touched where cus > 0."""
    import json
    from robust_e2e_gan_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    rows = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'conv_plan_table.json')))
    assert len(rows) == 468
    for args, want in rows:
        got = lib.conv_plan(*args[:13], flags=args[13], cus=256)
        assert got == want, (args, got, want)
        _check_conv_plan_is_built(got, args)
    so = lib.load()
    points = 0
    for cus in (64, 256, 0):          # 0: the chip re2e_conv_wgrad_workspace_bytes itself plans for (256 CUs without a device)
        for k, stride in ((3, 1), (4, 1), (4, 2)):
            for N, H, W in ((1, 5, 3), (2, 33, 8), (3, 21, 24), (32, 100, 40), (128, 800, 80)):
                if stride == 2 and (H % 2 or W % 2):
                    H, W = H + H % 2, W + W % 2
                for Cin, Cout in ((1, 64), (64, 1), (512, 1), (6, 10), (12, 20), (16, 64), (16, 192), (64, 64), (64, 128), (256, 512)):
                    for direction in (lib.CONV_FWD, lib.CONV_DGRAD, lib.CONV_WGRAD):
                        for extra in (0, lib.CONV_NO_WINOGRAD | lib.CONV_NO_WINO_WGRAD, lib.CONV_UNALIGNED, lib.CONV_MASK if direction == lib.CONV_DGRAD and
                                      stride == 1 else lib.CONV_POOL if direction == lib.CONV_FWD and k == 3 else 0):
                            act = _RELU if extra == lib.CONV_POOL else _NONE
                            plans = [lib.conv_plan(direction, N, H, W, Cin, Cout, k, k, stride, 1, act=act, flags=extra | f, cus=cus)
                                     for f in (0, lib.CONV_FILLER)]
                            for got, other in (plans, plans[::-1]):
                                where = (cus, direction, N, H, W, Cin, Cout, k, stride, extra, got)
                                points += 1
                                _check_conv_plan_is_built(got, where)
                                assert got['family'] == other['family'] and got['ws'] == other['ws'], where
                                if got['family'] == 'wino3x3':
                                    assert 1 <= int(got['images']) <= N and int(got['images']) * H * W * max(Cin, Cout) * 4 < 2 ** 31, where
                                if got.get('route', '').startswith('wgrad') and not extra & lib.CONV_UNALIGNED:
                                    # (the workspace is sized before there are pointers, for 16-byte aligned operands: an unaligned Cin == 1 /
                                    # Cout == 1 call goes to the engine, whose slice count may exceed the thin kernels' -- re2e_conv_wgrad then
                                    # answers "workspace too small", as before the plan existed)
                                    assert int(got['ws']) >= int(got['need']), where
                                    if cus == 0:
                                        OH, OW = (H + 2 - k) // stride + 1, (W + 2 - k) // stride + 1
                                        assert int(got['ws']) == so.re2e_conv_wgrad_workspace_bytes(N, OH, OW, Cin, Cout, k, k), where
    assert points == 3 * 3 * 5 * 10 * 3 * 4 * 2


def test_lm_plan_table():
    """re2e_lm_plan (the host functions re2e_lm_lstm_cell / _zo and re2e_lm_output choose their kernel form with) reads the addresses it is
    given and nothing behind them: on made-up addresses, without a device, the rows per trip, load widths and grid by row count, widths and
    alignment; what the calls refuse is refused."""
    from robust_e2e_gan_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    base = 1 << 20
    p = lib.lm_plan(lib.LM_PLAN_CELL, x=base, ldx=256, I=256, w_ih=base, w_hh=base, h_prev=base, n=12, H=650)
    assert p == dict(family='lm_cell', zo='0', rows='16', vi='4', vh='2', grid='650x1x1', block='128', trips='1'), p
    p = lib.lm_plan(lib.LM_PLAN_CELL, x=base + 4, ldx=8, I=8, w_ih=base, w_hh=base, h_prev=None, n=64, H=8)
    assert (p['rows'], p['vi'], p['vh'], p['trips']) == ('16', '1', '1', '4'), p
    p = lib.lm_plan(lib.LM_PLAN_CELL_ZO, w_hh=base, h_prev=base, n=5, H=8)          # no input: the pair falls to (1, 1)
    assert (p['zo'], p['rows'], p['vi'], p['vh']) == ('1', '8', '1', '1'), p
    p = lib.lm_plan(lib.LM_PLAN_OUTPUT, w_hh=base, h_prev=base + 8, n=4, H=12, V=4233)
    assert p == dict(family='lm_out', rows='4', vec='2', grid='1059x1x1', block='128', trips='1'), p
    for bad in (dict(n=0), dict(n=65), dict(ldx=7)):
        args = dict(x=base, ldx=8, I=8, w_ih=base, w_hh=base, h_prev=base, n=4, H=8)
        args.update(bad)
        with pytest.raises(lib.Re2eError):
            lib.lm_plan(lib.LM_PLAN_CELL, **args)
    with pytest.raises(lib.Re2eError):
        lib.lm_plan(lib.LM_PLAN_CELL, x=None, w_hh=base, n=4, H=8)                    # only the zoneout entry takes a cell without input
    with pytest.raises(lib.Re2eError):
        lib.lm_plan(3, w_hh=base, h_prev=base, n=4, H=8, V=5)


def test_missing_library_fails_loudly(monkeypatch):
    from robust_e2e_gan_amd import lib
    monkeypatch.setattr(lib, '_lib', None)
    monkeypatch.setattr(lib, 'LIB_PATH', '/nonexistent/libre2e_hip.so')
    with pytest.raises(lib.Re2eError):
        lib.load()


def test_ops_refuse_cpu_tensors():
    """The product path has no CPU fallback: CPU tensors raise instead of silently computing."""
    import torch
    from robust_e2e_gan_amd import ops, lib
    with pytest.raises(lib.Re2eError):
        ops.linear(torch.zeros(2, 3), torch.nn.Parameter(torch.zeros(4, 3)), None, None)
    with pytest.raises(lib.Re2eError):
        ops.mean_loss(torch.zeros(4), torch.zeros(4))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, 'robust_e2e_gan_amd')
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M), os.path.join(dp, f)
