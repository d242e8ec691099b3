"""Host side of Encoder.encode_batch (model/e2e_encoder.py): the per-layer heights the valid-height VGG stack hands its three Winograd layers,
and the grouping of a large batch.  The declaration of re2e_conv3x3_wino_valid itself -- header against library against lib.SIGNATURES -- is
covered by tests/test_abi.py as for every entry point; here only what ties it to its sibling.  No GPU."""
import os
import random
import re

from robust_e2e_gan_amd import lib
from robust_e2e_gan_amd.model.e2e_encoder import VGG2L, encode_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_valid_entry_point_takes_the_arguments_of_the_row_limited_one():
    """Same argument list as re2e_conv3x3_wino_rows, the per-image heights where that one takes its row limits."""
    assert lib.SIGNATURES['re2e_conv3x3_wino_valid'] == lib.SIGNATURES['re2e_conv3x3_wino_rows']
    header = open(os.path.join(ROOT, 'include', 're2e.h')).read()
    decl = {n: re.sub(r'\s+', ' ', re.search(r'int %s\(([^;]*)\);' % n, header).group(1)) for n in ('re2e_conv3x3_wino_valid', 're2e_conv3x3_wino_rows')}
    assert decl['re2e_conv3x3_wino_valid'] == decl['re2e_conv3x3_wino_rows'].replace('const int* row_lim', 'const int* valid_rows')


def test_valid_heights_follow_the_two_ceil_mode_pools():
    lens = list(range(1, 41))
    l1, l2, l3 = VGG2L.valid_heights(lens)
    assert l1 == lens
    assert l3 == VGG2L.pooled_lens(lens)
    for l, a, b in zip(lens, l2, l3):
        assert a == -(-l // 2) and b == -(-a // 2)
        assert 1 <= a <= (max(lens) + 1) // 2              # inside the pooled tensor's slot whatever the batch's longest utterance is
        # the last valid row of every layer is inside the rows the layer in front produced: a window of the pool reaches row 2 (a - 1) < l
        assert 2 * (a - 1) < l and 2 * (b - 1) < a


def test_groups_cover_every_utterance_once_and_go_back_in_place():
    rng = random.Random(3)
    for trial in range(200):
        U = rng.randint(1, 40)
        lens = [rng.randint(1, 40) for _ in range(U)]
        per = rng.randint(1, 45)
        groups = encode_groups(lens, per)
        seen = [u for idx, _ in groups for u in idx]
        assert sorted(seen) == list(range(U))
        assert all(1 <= len(idx) <= per for idx, _ in groups) and len(groups) == -(-U // per)
        for idx, T in groups:
            assert T == max(lens[u] for u in idx)
        if U <= per:
            assert groups == [(list(range(U)), max(lens))]          # one group: the caller's order, nothing to un-sort
        else:
            flat = [lens[u] for u in seen]
            assert flat == sorted(lens, reverse=True)               # longest first: a group pads to ITS longest utterance
            assert all(a < b for a, b in zip(seen, seen[1:]) if lens[a] == lens[b])          # ties in the caller's order
        # un-sort: results written at the indices land at the caller's positions
        back = [None] * U
        for idx, T in groups:
            for u, l in zip(idx, VGG2L.pooled_lens([lens[u] for u in idx])):
                back[u] = l
        assert back == VGG2L.pooled_lens(lens)
    assert encode_groups([5, 9, 7], 0) == [([1], 9), ([2], 7), ([0], 5)]             # a group holds at least one utterance
