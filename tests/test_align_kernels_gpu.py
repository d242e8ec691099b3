"""re2e_align_counts (csrc/align.hip) against the plain-Python restatement of its definition (tests/refs_align.py): counts and path bytes
exactly, for four cost vectors -- 4/3/3 (the default), 1/1/1 (Levenshtein), 2/3/1 (insertion != deletion: a swap of the two shows) and 7/3/3
(a substitution dearer than an insertion plus a deletion: never chosen).  The pairs: the two of the issue verbatim, every combination of the
lengths {0, 1, 2, 63, 64, 65, 127, 128, 129, 200} for reference x hypothesis over 3 symbols (many ties; strips of 64 rows and chunks of 64
columns start at 64 and 128; empty sides), one pair at the documented maximum of 1024 x 1024 labels, identical sequences and disjoint
alphabets.  The restatement of one cost vector's pairs is computed once (about 2 M cells) and shared by the tests that need it."""
import functools

import numpy as np
import pytest
import torch

import refs_align

gpu = pytest.mark.gpu
DEV = 'cuda:0'
COSTS = [(4, 3, 3), (1, 1, 1), (2, 3, 1), (7, 3, 3)]
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
MAX_LEN = 1024
VERBATIM = [([1, 1, 2, 2, 1], [3, 3, 3, 3, 3, 1, 2]), ([2, 3, 3, 1, 1, 1], [1, 1, 1, 3, 2, 3, 2])]


@functools.lru_cache(maxsize=None)
def _pairs():
    rng = np.random.default_rng(20240611)
    seq = lambda n, lo=1, hi=4: rng.integers(lo, hi, n).tolist()
    pairs = list(VERBATIM)
    pairs += [(seq(r), seq(h)) for r in LENGTHS for h in LENGTHS]
    pairs.append((seq(MAX_LEN), seq(MAX_LEN)))
    same = seq(70)
    pairs += [(same, list(same)), (seq(66), seq(67, 10, 13)), ([5], [5]), ([5], [6])]
    return pairs


@functools.lru_cache(maxsize=None)
def _want(costs):
    return [refs_align.align(r, h, costs) for r, h in _pairs()]


def _run(pairs, costs, pair_ref=None, refs=None):
    from robust_e2e_gan_amd.utils import score
    if refs is None:
        refs, pair_ref = [p[0] for p in pairs], list(range(len(pairs)))
    return score.align(refs, [p[1] for p in pairs], pair_ref, costs, paths=True, device=DEV)


@gpu
@pytest.mark.parametrize('costs', COSTS, ids=lambda c: '%d-%d-%d' % c)
def test_counts_and_paths_equal_the_restatement(costs):
    pairs, want = _pairs(), _want(costs)
    counts, paths = _run(pairs, costs)
    from robust_e2e_gan_amd.utils import score
    only_counts, none = score.align([p[0] for p in pairs], [p[1] for p in pairs], list(range(len(pairs))), costs, paths=False, device=DEV)
    assert none is None
    for k, ((ref, hyp), (c, p)) in enumerate(zip(pairs, want)):
        assert counts[k].tolist() == c, (k, len(ref), len(hyp), counts[k].tolist(), c)
        assert only_counts[k].tolist() == c, (k, len(ref), len(hyp), only_counts[k].tolist(), c)
        assert paths[k] == p, (k, len(ref), len(hyp))
    if costs == (4, 3, 3):
        assert counts[0].tolist() == [22, 6, 1, 4, 0, 2] and counts[1].tolist() == [21, 7, 3, 0, 3, 4]
    if costs == (1, 1, 1):
        assert counts[1].tolist()[1:] == [6, 1, 5, 0, 1]
    if costs == (7, 3, 3):
        assert int(counts[:, 3].sum()) == 0, 'a substitution at 7 was chosen over an insertion and a deletion at 3 + 3'


@gpu
def test_shared_references():
    """3 references x 4 hypotheses through pair_ref = 12 independent pairs."""
    rng = np.random.default_rng(5)
    refs = [rng.integers(1, 4, n).tolist() for n in (9, 70, 0)]
    hyps = [rng.integers(1, 4, n).tolist() for n in (0, 7, 66, 130)]
    pair_ref = [r for r in range(3) for _ in hyps]
    shared = _run([(None, h) for _ in range(3) for h in hyps], (4, 3, 3), pair_ref, refs)
    alone = _run([(refs[r], h) for r in range(3) for h in hyps], (4, 3, 3))
    assert (shared[0] == alone[0]).all() and shared[1] == alone[1]
    for k, r in enumerate(pair_ref):
        c, p = refs_align.align(refs[r], hyps[k % 4], (4, 3, 3))
        assert shared[0][k].tolist() == c and shared[1][k] == p, k


def _tables(pairs):
    from robust_e2e_gan_amd.utils import score
    ref_flat, ref_off = score.flat_table([p[0] for p in pairs])
    hyp_flat, hyp_off = score.flat_table([p[1] for p in pairs])
    cap = np.array([len(r) + len(h) for r, h in pairs], np.int64)
    path_off = np.concatenate([[0], np.cumsum(cap)]).astype(np.int64) + 64          # 64 sentinel bytes in front
    d = lambda a: torch.from_numpy(a).to(DEV)
    return d(ref_flat), ref_off, d(hyp_flat), hyp_off, np.arange(len(pairs), dtype=np.int32), path_off


@gpu
def test_write_footprint_and_determinism():
    """Sentinels around counts and around the path buffer stay; inside, every byte of a pair is written (the path, then zeros); a second
    call gives the same bytes."""
    from robust_e2e_gan_amd.utils import score
    pairs, want = _pairs(), _want((4, 3, 3))
    ref_d, ref_off, hyp_d, hyp_off, pair_ref, path_off = _tables(pairs)
    n = len(pairs)
    outs = []
    for _ in range(2):
        counts = torch.full((n + 2, 6), -777, dtype=torch.int32, device=DEV)
        path = torch.full((int(path_off[-1]) + 64,), 0xAB, dtype=torch.uint8, device=DEV)
        score.align_counts(ref_d, ref_off, hyp_d, hyp_off, pair_ref, (4, 3, 3), counts[1:n + 1], path, path_off)
        outs.append((counts.cpu().numpy(), path.cpu().numpy()))
    counts, path = outs[0]
    assert (counts[0] == -777).all() and (counts[-1] == -777).all()
    assert (path[:64] == 0xAB).all() and (path[int(path_off[-1]):] == 0xAB).all()
    for k, (c, p) in enumerate(want):
        got = path[int(path_off[k]):int(path_off[k + 1])].tobytes()
        assert counts[k + 1].tolist() == c and got == p.encode() + b'\0' * (len(got) - len(p)), k
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()


@gpu
def test_malformed_tables_are_rejected_on_the_host():
    """Each of a decreasing offset table, an out-of-range pair_ref, a cost of 0 or beyond the range and a sequence beyond the limit returns
    its error code and a message, and leaves the outputs untouched.  The checks run on the host before anything is enqueued: the calls are
    made with the tables as they are, and the outputs are read back afterwards."""
    from robust_e2e_gan_amd import lib
    from robust_e2e_gan_amd.utils import score
    so = lib.load()
    pairs = [([1, 2, 3], [1, 2]), ([2, 2], [3, 1, 1, 2]), ([1], [])]
    ref_d, ref_off, hyp_d, hyp_off, pair_ref, path_off = _tables(pairs)
    long_pairs = [([1] * (MAX_LEN + 1), [1, 2]), ([1, 2], [2] * (MAX_LEN + 1))]
    big = [_tables([p]) for p in long_pairs]
    counts = torch.full((3, 6), -777, dtype=torch.int32, device=DEV)
    path = torch.full((int(path_off[-1]) + 64 + 2 * MAX_LEN,), 0xAB, dtype=torch.uint8, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)

    def call(ref_d=ref_d, ref_off=ref_off, hyp_d=hyp_d, hyp_off=hyp_off, pair_ref=pair_ref, path_off=path_off, costs=(4, 3, 3)):
        rc = so.re2e_align_counts(ref_d.data_ptr(), ref_off.ctypes.data, len(ref_off) - 1, ref_d.numel(), hyp_d.data_ptr(), hyp_off.ctypes.data,
                                  pair_ref.ctypes.data, len(pair_ref), hyp_d.numel(), costs[0], costs[1], costs[2], counts.data_ptr(), path.data_ptr(),
                                  path_off.ctypes.data, path.numel(), ws.data_ptr(), ws.numel(), lib.stream())
        return rc, so.re2e_last_error().decode()

    bad = lambda a, i, v: np.concatenate([a[:i], [v], a[i + 1:]]).astype(a.dtype)
    EINVAL = -1
    cases = [(dict(ref_off=bad(ref_off, 1, 7)), EINVAL, 'ref_off'), (dict(hyp_off=bad(hyp_off, 2, 1)), EINVAL, 'hyp_off'),
             (dict(hyp_off=bad(hyp_off, 3, 99)), EINVAL, 'hyp_off'), (dict(pair_ref=bad(pair_ref, 1, 3)), EINVAL, 'pair_ref'),
             (dict(pair_ref=bad(pair_ref, 0, -1)), EINVAL, 'pair_ref'), (dict(costs=(0, 3, 3)), EINVAL, 'costs'),
             (dict(costs=(4, 256, 3)), EINVAL, 'costs'), (dict(costs=(4, 3, -2)), EINVAL, 'costs'),
             (dict(path_off=bad(path_off, 1, path_off[0] + 2)), EINVAL, 'path_off')]
    for t in big:
        cases.append((dict(ref_d=t[0], ref_off=t[1], hyp_d=t[2], hyp_off=t[3], pair_ref=t[4], path_off=t[5]), lib.EUNSUPPORTED, 'at most 1024'))
    for kw, code, word in cases:
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw.keys(), rc, msg)
        with pytest.raises(lib.Re2eError):
            score.align_counts(kw.get('ref_d', ref_d), kw.get('ref_off', ref_off), kw.get('hyp_d', hyp_d), kw.get('hyp_off', hyp_off),
                               kw.get('pair_ref', pair_ref), kw.get('costs', (4, 3, 3)), counts[:len(kw.get('pair_ref', pair_ref))], path,
                               kw.get('path_off', path_off))
    torch.cuda.synchronize()
    assert (counts.cpu() == -777).all() and (path.cpu() == 0xAB).all()
    rc, msg = call()                      # the same tables, well formed: served
    assert rc == 0, msg
    assert counts.cpu().numpy().tolist() == [refs_align.align(r, h)[0] for r, h in pairs]
