"""Plain-Python restatement of the alignment re2e_align_counts computes (include/re2e.h), and an independent two-row Levenshtein distance.

    D[0][0] = 0, D[i][0] = i deletions, D[0][j] = j insertions; cell (i, j) takes the best of, in this order, the diagonal (equal labels: a
    correct label at cost 0, else a substitution), a deletion from (i-1, j), an insertion from (i, j-1); best = the smallest (cost, errors)
    pair, compared lexicographically, the earlier candidate on a full tie.

Nothing here is shared with the kernel or with utils/score.py: cells are (cost, errors) tuples, the path is walked back over a table of
choices."""


def align(ref, hyp, costs=(4, 3, 3)):
    """-> ([cost, errors, C, S, D, I], path) with ``costs`` = (substitution, insertion, deletion) and ``path`` a str over 'CSDI' from the
    start of both sequences."""
    c_sub, c_ins, c_del = costs
    R, H = len(ref), len(hyp)
    cell = [[None] * (H + 1) for _ in range(R + 1)]
    how = [[None] * (H + 1) for _ in range(R + 1)]
    cell[0][0] = (0, 0)
    for i in range(1, R + 1):
        cell[i][0], how[i][0] = (i * c_del, i), 'D'
    for j in range(1, H + 1):
        cell[0][j], how[0][j] = (j * c_ins, j), 'I'
    for i in range(1, R + 1):
        for j in range(1, H + 1):
            d, u, l = cell[i - 1][j - 1], cell[i - 1][j], cell[i][j - 1]
            if ref[i - 1] == hyp[j - 1]:
                best, op = d, 'C'
            else:
                best, op = (d[0] + c_sub, d[1] + 1), 'S'
            cand = (u[0] + c_del, u[1] + 1)
            if cand < best:
                best, op = cand, 'D'
            cand = (l[0] + c_ins, l[1] + 1)
            if cand < best:
                best, op = cand, 'I'
            cell[i][j], how[i][j] = best, op
    i, j, path = R, H, []
    while i > 0 or j > 0:
        op = how[i][j]
        path.append(op)
        if op != 'I':
            i -= 1
        if op != 'D':
            j -= 1
    path = ''.join(reversed(path))
    n = {op: path.count(op) for op in 'CSDI'}
    assert n['S'] + n['D'] + n['I'] == cell[R][H][1]
    return [cell[R][H][0], cell[R][H][1], n['C'], n['S'], n['D'], n['I']], path


def levenshtein(a, b):
    """Edit distance with unit costs, two rows."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, y in enumerate(b, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y))
        prev = cur
    return prev[len(b)]


def replay(ref, hyp, path):
    """Walk ``path`` over both sequences: True when it consumes both exactly and every 'C' stands on equal labels, every 'S' on unequal ones."""
    i = j = 0
    for op in path:
        if op in 'CS':
            if i >= len(ref) or j >= len(hyp) or (ref[i] == hyp[j]) != (op == 'C'):
                return False
            i, j = i + 1, j + 1
        elif op == 'D':
            i += 1
        elif op == 'I':
            j += 1
        else:
            return False
    return i == len(ref) and j == len(hyp)
