"""k1mers2component as a brute force, written from the rule's text (oracle/partition.py:42-51: every k1-window of every contig adds
its partition to the set of the window's k1-mer), and the inputs that send shn_probe_build (csrc/probe_gpu.hip) down each of its
paths: k1-mers of one partition, of exactly two (pairs interned on the device), of three or more (interned on the host) and the
relaunch of that path's buffer.  Plain Python over strings: nothing here is shared with the kernels.

A case is (parts, k1, need): parts[p] = the contig strings of partition p (most partitions may be empty), need = what the brute
force must show of the input before the device is asked (see `require`), so that a case cannot miss the path it is named for."""
import random

import numpy as np


def expected_sets(parts, k1):
    """{k1-mer string: frozenset of the partitions it occurs in}"""
    sets = {}
    for p, contigs in enumerate(parts):
        for contig in contigs:
            for e in range(len(contig) - k1 + 1):
                sets.setdefault(contig[e:e + k1], set()).add(p)
    return {km: frozenset(s) for km, s in sets.items()}


def window_runs(parts, k1):
    """{k1-mer: the partition of each of its windows, partitions ascending, contig and position order inside one} -- the run of
    equal keys the device sees after its stable sort"""
    runs = {}
    for p, contigs in enumerate(parts):
        for contig in contigs:
            for e in range(len(contig) - k1 + 1):
                runs.setdefault(contig[e:e + k1], []).append(p)
    return {km: tuple(r) for km, r in runs.items()}


def key_of(km):
    """the 2-bit packing of a k1-mer, first base in the highest bits (A C G T = 0 1 2 3)"""
    v = 0
    for c in km:
        v = (v << 2) | "ACGT".index(c)
    return v


def flatten(parts):
    """the arguments of shn_probe_build: (text uint8[], off uint64[n + 1], part_of uint32[], n_contigs)"""
    flat = [c for contigs in parts for c in contigs]
    part_of = [p for p, contigs in enumerate(parts) for _c in contigs]
    joined = "".join(flat)
    text = np.frombuffer(joined.encode(), dtype=np.uint8).copy() if joined else np.zeros(1, np.uint8)
    off = np.zeros(len(flat) + 1, dtype=np.uint64)
    if flat:
        off[1:] = np.cumsum([len(c) for c in flat], dtype=np.uint64)
    return text, off, (np.array(part_of, dtype=np.uint32) if flat else np.zeros(1, np.uint32)), len(flat)


def require(parts, k1, need):
    """asserts the case's own precondition from the brute force.  need may hold:
      n1 / n2 / n3       at least so many k1-mers in one / exactly two / three or more partitions (0: exactly none)
      sets               frozensets that must each be the set of some k1-mer
      twice              sets that k1-mers of at least two different contigs must have
      lone               sets that exactly one k1-mer has
      shapes             runs (tuples of partitions, one per window) that must occur
      windows3           more than so many windows lie on k1-mers of three or more partitions
      n_keys             exactly so many distinct k1-mers
    Returns (sets, runs)."""
    sets, runs = expected_sets(parts, k1), window_runs(parts, k1)
    by_size = {1: 0, 2: 0, 3: 0}
    for s in sets.values():
        by_size[min(len(s), 3)] += 1
    for name, size in (("n1", 1), ("n2", 2), ("n3", 3)):
        if name in need:
            assert (by_size[size] == 0) if need[name] == 0 else (by_size[size] >= need[name]), (name, by_size)
    present = {}
    for km, s in sets.items():
        present.setdefault(s, []).append(km)
    for s in need.get("sets", ()):
        assert frozenset(s) in present, ("no k1-mer has the set", sorted(s))
    for s in need.get("lone", ()):
        assert len(present.get(frozenset(s), ())) == 1, ("not exactly one k1-mer with the set", sorted(s))
    for s in need.get("twice", ()):                              # (one contig per partition would be len(s) homes)
        kms = set(present.get(frozenset(s), ()))
        homes = set((p, ci) for p, contigs in enumerate(parts) for ci, contig in enumerate(contigs)
                    if any(contig[e:e + k1] in kms for e in range(len(contig) - k1 + 1)))
        assert len(homes) > len(s), ("the set is not reached from k1-mers of different contigs", sorted(s))
    shapes = set(runs.values())
    for sh in need.get("shapes", ()):
        assert tuple(sh) in shapes, ("no run shaped", sh)
    if "windows3" in need:
        w3 = sum(len(r) for km, r in runs.items() if len(sets[km]) >= 3)
        assert w3 > need["windows3"], w3
    if "n_keys" in need:
        assert len(sets) == need["n_keys"], len(sets)
    return sets, runs


# ---- builders

def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


class _Planter(object):
    """contigs of random bases around planted segments.  Every copy of a segment gets flanks of its own: the base before and the
    base after differ from copy to copy (cycled through the four bases -- up to four copies differ pairwise), so copies share
    the segment's k1-mers and no other."""

    def __init__(self, n_parts, seed, flank=60):
        self.rng = random.Random(seed)
        self.parts = [[] for _ in range(n_parts)]
        self.flank = flank

    def segment(self, n):
        return _rand(self.rng, n)

    def plant(self, seg, where, bare=False):
        """one contig holding seg in every partition of `where` (a partition named twice gets two contigs); bare: the contig IS
        the segment (more than four copies: flanks could no longer differ pairwise)"""
        for i, p in enumerate(where):
            if bare:
                self.parts[p].append(seg)
                continue
            left, right = "ACGT"[i % 4], "TGCA"[(i // 4 + i) % 4]
            self.parts[p].append(_rand(self.rng, self.flank) + left + seg + right + _rand(self.rng, self.flank))

    def filler(self, p, n=150):
        self.parts[p].append(_rand(self.rng, n))


def single_repeat_in_contig(k1=21):
    """a k1-mer twice inside one contig; every k1-mer in one partition"""
    pl = _Planter(3, 101)
    seg = pl.segment(k1 + 5)
    pl.filler(0)
    pl.parts[1].append(_rand(pl.rng, 70) + "A" + seg + "C" + _rand(pl.rng, 40) + "G" + seg + "T" + _rand(pl.rng, 70))
    pl.filler(2)
    return pl.parts, k1, {"n1": 300, "n2": 0, "n3": 0, "shapes": [(1, 1)]}


def single_shared_in_partition(k1=21):
    """a k1-mer on two contigs (and a second on three) of ONE partition: runs longer than 1 that are not multi"""
    pl = _Planter(4, 102)
    pl.plant(pl.segment(k1 + 30), [2, 2])
    pl.plant(pl.segment(k1), [0, 0, 0])
    pl.filler(1)
    pl.filler(3)
    return pl.parts, k1, {"n1": 300, "n2": 0, "n3": 0, "shapes": [(2, 2), (0, 0, 0)]}


# (the smaller partition of a pair lies in the top bits of the sorted word and is n_parts - 2 at the most: at 258 and 65,538 the
# pair (n_parts - 2, n_parts - 1) sets the highest bit of the range, which shn_bits_for widened one partition earlier)
PAIR_N_PARTS = (2, 3, 255, 256, 257, 258, 65537, 65538)


def pairs(n_parts, k1=21):
    """k1-mers of exactly two partitions: the pairs at the ends of the partition range (the highest partition numbers carry the
    top bits of the pair sort's range, 32 + shn_bits_for(n_parts)), many k1-mers on a pair and one alone on a pair, runs of three
    windows over two partitions in both shapes"""
    pl = _Planter(n_parts, 200 + n_parts)
    last = n_parts - 1
    want = [(0, 1), (0, last), (max(last - 1, 0), last)]
    if n_parts >= 4:
        want += [(1, last - 1), (n_parts // 2, n_parts // 2 + 1)]
    want = sorted(set(p for p in want if p[0] != p[1]))
    lone = []
    if n_parts == 3:                                            # (three partitions have three pairs: (0, 2) is the lone one)
        want, lone = [(0, 1), (1, 2)], [(0, 2)]
    elif n_parts > 3:
        lone = [(1, last)]
    assert not set(lone) & set(want)
    for pr in want:
        pl.plant(pl.segment(k1 + 40), pr)                       # 41 k1-mers on the pair
        pl.plant(pl.segment(k1 + 7), pr)                        # ... and 8 more from other contigs: the same set id
    for pr in lone:                                             # a pair that a single k1-mer has
        pl.plant(pl.segment(k1), pr)
    p, q = want[0]
    pl.plant(pl.segment(k1 + 3), (p, p, q))
    p, q = want[-1]
    pl.plant(pl.segment(k1 + 3), (p, q, q))
    pl.filler(0)
    need = {"n1": 100, "n2": 49 * len(want) + 8, "n3": 0, "sets": want + lone, "twice": want, "lone": lone,
            "shapes": [(want[0][0], want[0][0], want[0][1]), (want[-1][0], want[-1][1], want[-1][1])]}
    return pl.parts, k1, need


def multi(k1=21):
    """k1-mers of 3, 4 and 40 partitions, one set from different contigs, a run (p, q, q, r); no k1-mer of exactly two"""
    pl = _Planter(48, 301)
    three, four, forty = (1, 5, 9), (0, 2, 3, 47), tuple(range(3, 43))
    pl.plant(pl.segment(k1 + 25), three)
    pl.plant(pl.segment(k1 + 4), three)                         # the same set from other contigs: one id
    pl.plant(pl.segment(k1 + 10), four)
    pl.plant(pl.segment(k1 + 2), forty, bare=True)
    pl.plant(pl.segment(k1 + 6), (6, 8, 8, 30))
    pl.filler(46)
    need = {"n1": 100, "n2": 0, "n3": 26 + 5 + 11 + 3 + 7, "sets": [three, four, forty, (6, 8, 30)], "twice": [three],
            "shapes": [(6, 8, 8, 30), forty]}
    return pl.parts, k1, need


def mixed(k1, seed=401):
    """k1-mers of one, of two and of three or more partitions in one call, sets shared between contigs on both multi paths"""
    pl = _Planter(7, seed + k1)
    pl.plant(pl.segment(k1 + 20), (0, 1))
    pl.plant(pl.segment(k1 + 5), (0, 1))
    pl.plant(pl.segment(k1 + 12), (2, 6))
    pl.plant(pl.segment(k1), (5, 6))
    pl.plant(pl.segment(k1 + 15), (0, 3, 6))
    pl.plant(pl.segment(k1 + 3), (0, 3, 6))
    pl.plant(pl.segment(k1 + 8), (1, 2, 4, 5))
    pl.plant(pl.segment(k1 + 2), (1, 1, 4))
    pl.plant(pl.segment(k1 + 2), (2, 3, 3, 5))
    for p in range(7):
        pl.filler(p, 120)
    need = {"n1": 500, "n2": 21 + 6 + 13 + 1 + 3, "n3": 16 + 4 + 9 + 3,
            "sets": [(0, 1), (2, 6), (5, 6), (0, 3, 6), (1, 2, 4, 5), (1, 4), (2, 3, 5)], "twice": [(0, 1), (0, 3, 6)], "lone": [(5, 6)],
            "shapes": [(1, 1, 4), (2, 3, 3, 5)]}
    return pl.parts, k1, need


def relaunch(k1=21):
    """one segment of 22,000 windows in three partitions: 66,000 windows for the host path, above the 65,536 its buffer starts
    with -- the kernel runs a second time with the room it asked for"""
    pl = _Planter(5, 501, flank=30)
    pl.plant(pl.segment(22000 + k1 - 1), (0, 2, 4))
    pl.plant(pl.segment(k1 + 9), (1, 3))
    pl.plant(pl.segment(k1 + 4), (1, 2, 3))
    return pl.parts, k1, {"windows3": 1 << 16, "n3": 22000 + 5, "n2": 10, "n1": 100, "sets": [(0, 2, 4), (1, 3), (1, 2, 3)]}


def width_2():
    """k1 = 2: sixteen keys at the most, in runs of hundreds of windows"""
    rng = random.Random(601)
    parts = [[_rand(rng, 900), _rand(rng, 600)], [_rand(rng, 1000, "AC")], [_rand(rng, 700, "AT"), "GG"], ["G" * 50, "C"], [_rand(rng, 400, "CG")]]
    return parts, 2, {"n_keys": 16, "n2": 1, "n3": 3, "sets": [(0,), (0, 1, 2), (0, 1, 4)]}


def width_32_poly():
    """k1 = 32 (the key fills the word): the all-ones key (poly-T) and the all-zero key (poly-A), alone and shared.  The table is
    not canonical: T...T and A...A are two k1-mers."""
    pl = _Planter(6, 602)
    pl.parts[0].append("A" * 40)
    pl.parts[1].append("T" * 32)
    pl.parts[4].append("T" * 45)
    pl.parts[5].append("C" * 33)
    pl.parts[2].append("G" * 32)
    pl.parts[3].append("G" * 34)
    pl.parts[5].append("G" * 32)
    pl.plant(pl.segment(32 + 6), (0, 5))
    for p in range(6):
        pl.filler(p, 100)
    parts, k1 = pl.parts, 32
    need = {"n1": 300, "n2": 8, "n3": 1, "sets": [(0,), (1, 4), (5,), (2, 3, 5), (0, 5)], "shapes": [(0,) * 9, (1,) + (4,) * 14]}
    return parts, k1, need


def degenerate_lengths(k1=21):
    """contigs shorter than k1, of exactly k1 bases and empty ones among ordinary ones"""
    rng = random.Random(701)
    exact = _rand(rng, k1)
    parts = [["", _rand(rng, k1 - 1), _rand(rng, 90)], [exact, "", ""], [_rand(rng, 1), "G" + exact[:-1] + ("A" if exact[-1] != "A" else "C"), _rand(rng, 80), ""], [exact]]
    return parts, k1, {"n1": 70 + 60 + 1, "sets": [(1, 3)], "lone": [(1, 3)], "n3": 0}


def no_window(k1=21):
    rng = random.Random(702)
    return [[_rand(rng, k1 - 1), "A"], [], [_rand(rng, 5), "", _rand(rng, k1 - 1)]], k1, {"n_keys": 0}


def all_empty(k1=21):
    return [["", ""], [""], []], k1, {"n_keys": 0}


def no_contig(k1=21):
    return [[], [], []], k1, {"n_keys": 0}


def empty_ends(k1=21):
    """the first and the last partitions have no contig"""
    pl = _Planter(9, 703)
    pl.plant(pl.segment(k1 + 9), (2, 6))
    pl.plant(pl.segment(k1 + 1), (2, 4, 6))
    pl.filler(3)
    assert not pl.parts[0] and not pl.parts[1] and not pl.parts[7] and not pl.parts[8]
    return pl.parts, k1, {"n1": 100, "n2": 10, "n3": 2, "sets": [(2, 6), (2, 4, 6)]}


def reads_from(parts, n, length, seed):
    """n reads of `length` bases drawn from the contigs long enough for one, every other one reverse-complemented, and a few of
    random bases that hit nothing"""
    rng = random.Random(seed)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    long_enough = [c for contigs in parts for c in contigs if len(c) >= length]
    out = []
    for i in range(n):
        if i % 10 == 9:
            out.append(_rand(rng, length))
            continue
        c = long_enough[rng.randrange(len(long_enough))]
        at = rng.randrange(len(c) - length + 1)
        r = c[at:at + length]
        out.append("".join(comp[b] for b in reversed(r)) if i % 2 else r)
    return out
