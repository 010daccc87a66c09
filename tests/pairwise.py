"""The greedy pairwise covering set that the pipeline's chain tests draw their cases from (tests/test_pipeline_chain_gpu.py,
tests/pipeline3d_cases.py).  Deterministic: the same factors give the same cases in the same order."""
import itertools


def pairwise_cases(factors):
    """A greedy covering set: each new case starts from the first uncovered pair and gives every other factor the level
    (first on ties) that covers the most still uncovered pairs with the levels chosen so far.  Levels are indices."""
    names = list(factors)
    uncovered = {(a, i, b, j) for x, a in enumerate(names) for b in names[x + 1:]
                 for i in range(len(factors[a])) for j in range(len(factors[b]))}
    order = {n: k for k, n in enumerate(names)}

    def key(m, lm, n, ln):
        return (m, lm, n, ln) if order[m] < order[n] else (n, ln, m, lm)

    cases = []
    while uncovered:
        a, i, b, j = min(uncovered, key=lambda p: (order[p[0]], p[1], order[p[2]], p[3]))
        case = {a: i, b: j}
        for n in names:
            if n not in case:
                case[n] = max(range(len(factors[n])),
                              key=lambda k: (sum(key(m, case[m], n, k) in uncovered for m in case), -k))
        uncovered -= {key(m, case[m], n, case[n]) for m, n in itertools.combinations(names, 2)}
        cases.append({n: factors[n][case[n]] for n in names})
    return cases


def uncovered_pairs(factors, cases):
    """The (factor, level, factor, level) pairs that no case of `cases` (dicts of levels) has."""
    names = list(factors)
    covered = {(a, c[a], b, c[b]) for c in cases for i, a in enumerate(names) for b in names[i + 1:]}
    return [(a, la, b, lb) for x, a in enumerate(names) for b in names[x + 1:]
            for la, lb in itertools.product(factors[a], factors[b]) if (a, la, b, lb) not in covered]
