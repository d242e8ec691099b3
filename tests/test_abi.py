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
