"""shn_cc_solve (csrc/components.hip: the lock-free union-find over the edges between owner shards) alone, against scipy's
connected components: the distinct ids ascending, for each the smallest id of its component, n_nodes = the number of distinct ids.
Deep trees (long chains in every edge order), stars, forests, repeated edges, self-loops, the empty edge list; 64-bit ids below,
across and above 2^32, with id_limit unknown (0), exact, and exactly at the digit edges of the sort.  Every graph is solved twice --
as given, and with the edges permuted and their ends swapped -- and both answers must be the reference's.  All comparisons exact;
every shape runs once."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -0x0123456789ABCDEF


@pytest.fixture(scope="module")
def ctx():
    from shannon_amd import device
    c = device.Context(0)
    yield c
    c.close()


def reference(edges):
    """(distinct ids ascending, the smallest id of each one's component) by scipy on the ids compacted with np.unique"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    edges = np.asarray(edges, dtype=np.uint64).reshape(-1, 2)
    ids, inv = np.unique(edges.reshape(-1), return_inverse=True)
    inv = inv.reshape(-1, 2)
    n = len(ids)
    _, comp = connected_components(coo_matrix((np.ones(len(inv), np.int8), (inv[:, 0], inv[:, 1])), shape=(n, n)), directed=False)
    first = np.full(comp.max() + 1, n, dtype=np.int64)
    np.minimum.at(first, comp, np.arange(n))                         # (compact numbers follow the ids: the smallest number is the smallest id)
    return ids, ids[first[comp]]


def solve(ctx, edges, id_limit):
    """one shn_cc_solve: (ids, labels) as uint64 arrays of n_nodes entries; what lies behind them in the buffers is left alone"""
    import torch
    from shannon_amd import device
    edges = np.ascontiguousarray(np.asarray(edges, dtype=np.uint64).reshape(-1, 2))
    E = len(edges)
    ge = torch.as_tensor(edges.view(np.int64).reshape(-1).copy(), device="cuda") if E else torch.zeros(2, dtype=torch.int64, device="cuda")
    nodes = torch.full((2 * max(E, 1),), SENTINEL, dtype=torch.int64, device="cuda")
    labels = torch.full((2 * max(E, 1),), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    nn = device.ComponentShards.solve(ctx, ge.data_ptr(), E, int(id_limit), nodes.data_ptr(), labels.data_ptr())
    assert 0 <= nn <= 2 * E
    assert (nodes[nn:] == SENTINEL).all() and (labels[nn:] == SENTINEL).all(), "written behind n_nodes"
    return nodes[:nn].cpu().numpy().view(np.uint64), labels[:nn].cpu().numpy().view(np.uint64)


def check(ctx, edges, id_limit=None, seed=5):
    """both solves (as given; permuted with the ends swapped) against the reference.  id_limit None: the largest id + 1."""
    edges = np.asarray(edges, dtype=np.uint64).reshape(-1, 2)
    want_ids, want_labels = reference(edges)
    if id_limit is None:
        id_limit = int(edges.max()) + 1
    assert id_limit == 0 or int(edges.max()) < id_limit
    rng = np.random.default_rng(seed)
    other = edges[rng.permutation(len(edges))][:, ::-1]
    for what, e in (("as given", edges), ("permuted and swapped", other)):
        ids, labels = solve(ctx, e, id_limit)
        assert len(ids) == len(want_ids), (what, len(ids), len(want_ids))
        assert np.array_equal(ids, want_ids), what
        bad = np.nonzero(labels != want_labels)[0]
        assert len(bad) == 0, "%s: %d of %d labels wrong, the first: id %d got %d want %d" % (
            what, len(bad), len(ids), ids[bad[0]], labels[bad[0]], want_labels[bad[0]])
    return want_ids, want_labels


def u64(x):
    return np.array(x, dtype=np.uint64).reshape(-1, 2)


def chain(n, lo=0):
    a = np.arange(lo, lo + n - 1, dtype=np.uint64)
    return np.stack([a, a + np.uint64(1)], axis=1)


def forest(n, length, lo=0):
    """chains of `length` nodes over the ids lo .. lo + n - 1"""
    a = np.arange(n - 1, dtype=np.uint64)
    a = a[(a % np.uint64(length)) != np.uint64(length - 1)] + np.uint64(lo)
    return np.stack([a, a + np.uint64(1)], axis=1)


# ---- deep trees

@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_one_chain_of_100000_nodes(ctx, order):
    e = chain(100000)
    if order == "descending":
        e = e[::-1]
    elif order == "shuffled":
        e = e[np.random.default_rng(1).permutation(len(e))]
    ids, labels = check(ctx, e)
    assert len(ids) == 100000 and (labels == 0).all()


def test_forest_of_chains_of_1000(ctx):
    ids, labels = check(ctx, forest(100000, 1000))
    assert len(np.unique(labels)) == 100 and np.array_equal(labels, ids - ids % np.uint64(1000))


@pytest.mark.parametrize("centre", ["largest", "smallest"])
def test_star(ctx, centre):
    n = 50000
    leaves = np.arange(1, n, dtype=np.uint64) if centre == "smallest" else np.arange(0, n - 1, dtype=np.uint64)
    c = np.uint64(0 if centre == "smallest" else n - 1)
    e = np.stack([np.full(n - 1, c, dtype=np.uint64), leaves], axis=1)
    ids, labels = check(ctx, e)
    assert len(ids) == n and (labels == 0).all()


def test_random_sparse_graph(ctx):
    """about one edge per two nodes: many small components, ids with gaps (nodes without an edge are not nodes)"""
    rng = np.random.default_rng(2)
    e = rng.integers(0, 200000, size=(100000, 2)).astype(np.uint64)
    ids, labels = check(ctx, e)
    assert len(ids) < 200000 and 1000 < len(np.unique(labels)) < len(ids)


def test_every_edge_repeated(ctx):
    rng = np.random.default_rng(3)
    e = rng.integers(0, 40000, size=(20000, 2)).astype(np.uint64)
    ids1, labels1 = reference(e)
    ids, labels = check(ctx, np.concatenate([e, e[::-1], e[:, ::-1], e, e]))
    assert np.array_equal(ids, ids1) and np.array_equal(labels, labels1)


def test_self_loops(ctx):
    """(u, u) on nodes of a component, and a node that appears only in a self-loop: a node, its own label"""
    e = np.concatenate([chain(50, 10), u64([[20, 20], [10, 10], [59, 59]]), u64([[7, 7]]), u64([[1000, 1000], [1000, 1000]]), chain(5, 200), u64([[204, 204]])])
    ids, labels = check(ctx, e)
    lab = dict(zip(ids.tolist(), labels.tolist()))
    assert lab[7] == 7 and lab[1000] == 1000 and lab[59] == 10 and lab[204] == 200 and len(ids) == 50 + 1 + 1 + 5


def test_a_single_edge_and_a_single_self_loop(ctx):
    ids, labels = check(ctx, [[9, 4]])
    assert ids.tolist() == [4, 9] and labels.tolist() == [4, 4]
    ids, labels = check(ctx, [[6, 6]])
    assert ids.tolist() == [6] and labels.tolist() == [6]


def test_no_edge(ctx):
    """n_edges == 0: n_nodes is 0 and nothing is written (solve() checks the buffers behind n_nodes: here all of them)"""
    for id_limit in (0, 1, 1 << 40):
        ids, labels = solve(ctx, np.zeros((0, 2), np.uint64), id_limit)
        assert len(ids) == 0 and len(labels) == 0


# ---- id width

def chain_and_forest(shift):
    """a chain of 20,000, chains of 1,000 over 30,000 more ids and a few links between chains, all ids shifted"""
    e = np.concatenate([chain(20000), forest(30000, 1000, 20000), u64([[20500, 31700], [49999, 3], [25000, 25000]])])
    return e + np.uint64(shift)


@pytest.mark.parametrize("limit", ["unknown", "exact"])
@pytest.mark.parametrize("shift", [0, 2 ** 32 - 50, 2 ** 40, 2 ** 61], ids=["below_2^32", "straddling_2^32", "above_2^32_at_2^40", "above_2^32_at_2^61"])
def test_ids_below_across_and_above_2_32(ctx, shift, limit):
    e = chain_and_forest(shift)
    lo, hi = int(e.min()), int(e.max())
    assert lo == shift and hi == shift + 49999
    if shift == 2 ** 32 - 50:
        assert lo < 2 ** 32 <= hi
    elif shift:
        assert lo >= 2 ** 32
    else:
        assert hi < 2 ** 32
    ids, labels = check(ctx, e, id_limit=0 if limit == "unknown" else hi + 1)
    # the same partition as without the shift, the labels shifted with the ids
    ids0, labels0 = reference(chain_and_forest(0))
    assert np.array_equal(ids - np.uint64(shift), ids0) and np.array_equal(labels - np.uint64(shift), labels0)
    assert len(np.unique(labels)) == 1 + 30 - 2                      # (the chain + 30 chains; two links join, the third is a self-loop)


@pytest.mark.parametrize("id_limit", [255, 256, 257, 65536, 2 ** 32, 2 ** 32 + 1])
def test_id_limit_at_the_digit_edges_of_the_sort(ctx, id_limit):
    """the sort goes over the bits of id_limit in steps of 8; the largest id present is id_limit - 1 and hangs on a chain that
    ends at a small id: its label is that id"""
    rng = np.random.default_rng(id_limit % 1000)
    top = id_limit - 1
    small = 3
    mids = np.unique(rng.integers(small + 1, top, size=40).astype(np.uint64))
    path = np.concatenate([np.array([small], np.uint64), mids, np.array([top], np.uint64)])      # small - ... - top, ascending ids
    others = rng.integers(0, id_limit, size=(300, 2)).astype(np.uint64)
    path_e = np.stack([path[:-1], path[1:]], axis=1)
    e = np.concatenate([others, path_e[::-1]])
    assert e.dtype == np.uint64 and int(e.max()) == top
    ids, labels = check(ctx, e, id_limit=id_limit)
    assert int(ids[-1]) == top
    assert int(labels[-1]) == int(reference(e)[1][-1]) <= small       # (a random edge may lead on to 0, 1 or 2)
