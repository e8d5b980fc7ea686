"""The merge of class sets as a brute force, written from the rule's text: every class of every part is a weighted list;
the merged classes are one per distinct list, its weight the sum of that list's weights, in ascending order of the list's 63-bit key
(shannon_amd.abundance.list_key: plain integers, no library).  Two different lists with one key would keep their order of arrival."""
import numpy as np


def brute_merge(lists, weights):
    """[(list as a tuple, summed weight)] in ascending key order"""
    from shannon_amd import abundance
    total = {}
    for M, w in zip(lists, weights):
        M = tuple(int(j) for j in M)
        assert M and list(M) == sorted(set(M)), "a list is ascending, distinct, not empty"
        total[M] = total.get(M, 0) + int(w)                   # (a dict keeps the order of first arrival)
    return sorted(total.items(), key=lambda kv: abundance.list_key(kv[0]))


def csr(lists):
    """(class_off uint64[n + 1], members uint32[]) of lists one after the other"""
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    if lists:
        off[1:] = np.cumsum([len(M) for M in lists], dtype=np.uint64)
    return off, np.array([j for M in lists for j in M], dtype=np.uint32)


def brute_arrays(lists, weights):
    """the brute force as the arrays an export holds: (class_off, members, n_c)"""
    merged = brute_merge(lists, weights)
    off, mem = csr([M for M, _w in merged])
    return off, mem, np.array([w for _M, w in merged], dtype=np.uint64)


def lists_of(cl):
    """the classes of a class dict as [(tuple, n_c)]"""
    off = [int(x) for x in cl["class_off"]]
    return [(tuple(int(j) for j in cl["members"][off[c]:off[c + 1]]), int(n)) for c, n in enumerate(cl["n_c"])]
