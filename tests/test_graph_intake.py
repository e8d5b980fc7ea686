"""shannon_amd/graph_intake.py: which form a partition's reads take to the native graph stage, from plain values, and the retry with
the k1-mer rows.  No device call."""
import numpy as np
import pytest

from shannon_amd import graph_intake as gi
from shannon_amd._lib import ShannonError

# (native_graph, rows_mode, routes_on_device, check_rows, ss, n_routed) -> form, for the flag combinations that reach each form
CASES = [
    ((True, True, True, None, False, 100), gi.ROWS_BY_PLACE),       # code matrices + GPU unitigs, the routes left on the device
    ((True, True, True, None, False, 1), gi.ROWS_BY_PLACE),
    ((True, True, True, "1", False, 100), gi.ROWS),                 # SHN_GRAPH_CHECK wants the indices on the host: by place off
    ((True, True, False, None, False, 100), gi.ROWS),               # the routes fetched to the host
    ((True, True, False, "1", False, 100), gi.ROWS),
    ((True, True, True, None, False, 0), gi.GATHERED),              # a by-place partition without a read falls back
    ((True, True, True, "1", False, 0), gi.GATHERED),
    ((True, True, False, None, False, 0), gi.GATHERED),
    ((True, False, False, None, False, 100), gi.GATHERED),          # reads as strings, SHN_GRAPH_ROWS=0, no GPU unitigs, two mate lengths
    ((True, False, True, None, False, 100), gi.GATHERED),           # (routes left on the device for a rows mode the back half then declines)
    ((True, False, False, "1", False, 100), gi.GATHERED),
    ((True, False, False, None, True, 100), gi.GATHERED),           # -s never takes a rows form
    ((True, True, True, None, True, 100), gi.GATHERED),
    ((True, False, False, None, True, 0), gi.GATHERED),
    ((False, False, False, None, False, 100), gi.PYTHON),           # native_graph=False
    ((False, True, True, None, False, 100), gi.PYTHON),
    ((False, False, False, None, True, 100), gi.PYTHON),
    ((False, False, False, "1", False, 0), gi.PYTHON),
]


@pytest.mark.parametrize("args, form", CASES)
def test_choose_form(args, form):
    assert gi.choose_form(*args) == form


def test_the_four_forms_are_four_names():
    assert len({gi.ROWS_BY_PLACE, gi.ROWS, gi.GATHERED, gi.PYTHON}) == 4


class _Store(object):
    def __init__(self, r1, r2=None):
        self.r1, self.r2 = r1, r2


def test_rows_possible(monkeypatch):
    monkeypatch.delenv("SHN_GRAPH_ROWS", raising=False)
    m = np.zeros((4, 50), np.uint8)
    dev = object()
    assert gi.is_code_matrix(m)
    for no in (m.T, m[:, ::2], m.astype(np.int8), m[0], ["ACGT"] * 4, None):
        assert not gi.is_code_matrix(no)
    assert gi.rows_possible(_Store(m), dev, None, False, False)
    assert gi.rows_possible(_Store(m, m), dev, dev, True, False)
    assert not gi.rows_possible(_Store(m, m), dev, dev, True, True)                 # -s
    assert not gi.rows_possible(_Store(m, m), dev, None, True, False)               # second mates not resident
    assert not gi.rows_possible(_Store(m, ["ACGT"] * 4), dev, dev, True, False)
    assert not gi.rows_possible(_Store(["ACGT"] * 4), dev, None, False, False)
    assert not gi.rows_possible(_Store(m), None, None, False, False)
    monkeypatch.setenv("SHN_GRAPH_ROWS", "0")
    assert not gi.rows_possible(_Store(m), dev, None, False, False)


ROWS = np.arange(26, dtype=np.uint8)
MARKED = "shn_mbgraph_run_unitigs: cyclic partition needs the k1-mer rows (code -1)"


def _part(made):
    def make():
        made.append(1)
        return ROWS
    return {"k1mer_bytes": {"lazy": make, "kept": ROWS}}


def test_retry_not_needed():
    seen, made = [], []
    assert gi.with_k1mer_rows(lambda rb: seen.append(rb) or "graph", _part(made), "lazy") == "graph"
    assert seen == [None] and not made


@pytest.mark.parametrize("name", ["lazy", "kept"])
def test_retry_with_the_rows(name):
    seen, made = [], []

    def call(rb):
        seen.append(rb)
        if rb is None:
            raise ShannonError(MARKED)
        return "graph"
    assert gi.with_k1mer_rows(call, _part(made), name) == "graph"
    assert len(seen) == 2 and seen[0] is None and seen[1] is ROWS and len(made) == (name == "lazy")


def test_other_errors_and_a_second_refusal_propagate():
    seen, made = [], []

    def other(rb):
        seen.append(rb)
        raise ShannonError("shn_mbgraph_run_rows: out of device memory (code -2)")
    with pytest.raises(ShannonError, match="out of device memory"):
        gi.with_k1mer_rows(other, _part(made), "lazy")
    assert seen == [None] and not made

    def marked(rb):
        seen.append(rb)
        raise ShannonError(MARKED)
    del seen[:]
    with pytest.raises(ShannonError, match="needs the k1-mer rows"):
        gi.with_k1mer_rows(marked, _part(made), "lazy", ROWS)               # rows already given: no second call
    assert len(seen) == 1 and seen[0] is ROWS and not made
    del seen[:]
    with pytest.raises(ShannonError, match="needs the k1-mer rows"):
        gi.with_k1mer_rows(marked, _part(made), "lazy")                     # refused again with the rows: no third call
    assert len(seen) == 2 and seen[1] is ROWS
