"""The brute-force statement of the pattern mining rule — the yardstick of dr4sr_amd.mine, kept as plain as it can be.

A pattern is a tuple of k ids, 2 <= k <= alpha.  It occurs in a sequence s if there are positions p_0 < p_1 < ... < p_{k-1} with
s[p_i] = t_i and p_{k-1} - p_0 <= alpha - 1: all of its items lie inside a window of alpha consecutive positions.  Its frequency is the
number of sequences with at least one occurrence.  The result is every pattern with frequency >= beta as [id_0, ..., id_{k-1}, frequency],
frequency descending, then id tuple ascending (a tuple that is a prefix of another comes first: Python's tuple order)."""
import collections
import itertools


def brute_force(sequences, alpha=5, beta=2):
    count = collections.Counter()
    for s in sequences:
        seen = set()
        for p in range(len(s)):
            later = range(p + 1, min(len(s), p + alpha))            # the positions at most alpha - 1 after p
            for n in range(1, len(later) + 1):
                for rest in itertools.combinations(later, n):
                    seen.add((s[p],) + tuple(s[q] for q in rest))
        count.update(seen)
    kept = sorted((-f, t) for t, f in count.items() if f >= beta)
    return [[int(v) for v in t] + [int(-f)] for f, t in kept]
