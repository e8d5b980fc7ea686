"""How a partition's reads reach the native graph stage, decided from plain values (the Python side of choose_intake / IntakeForm
in csrc/mbgraph_host.hip), and the one retry every caller of that stage shares.  No device call is made here."""
import os
import numpy as np
from ._lib import ShannonError

ROWS_BY_PLACE = "rows by place"     # the reads named by their place in the routes left on the device
ROWS = "rows"                       # the reads named by an index array into the resident code matrices
GATHERED = "gathered"               # the reads' codes gathered on the host (every -s run; SHN_GRAPH_ROWS=0; stores that are no matrices)
PYTHON = "python"                   # mbgraph.run_partition, native_graph=False


def is_code_matrix(m):
    return isinstance(m, np.ndarray) and m.dtype == np.uint8 and m.ndim == 2 and m.flags["C_CONTIGUOUS"]


def rows_possible(store, d1, d2, paired, ss):
    """the reads are resident on the device AND kept on the host as C-contiguous uint8 code matrices, double-stranded, SHN_GRAPH_ROWS
    not 0: the rows forms may name them.  (-s hands the reads over as gathered rows + strand flags: the rows forms know the doubled
    layout only.)"""
    return (d1 is not None and is_code_matrix(getattr(store, "r1", None)) and
            (not paired or (d2 is not None and is_code_matrix(getattr(store, "r2", None)))) and
            os.environ.get("SHN_GRAPH_ROWS", "1") != "0" and not ss)


def choose_form(native_graph, rows_mode, routes_on_device, check_rows, ss, n_routed):
    """the form one partition takes.  routes_on_device: its routes are a RouteView into the device routes; check_rows:
    SHN_GRAPH_CHECK is set (the check wants the indices on the host); n_routed: its routed reads after the cutoff."""
    if not native_graph:
        return PYTHON
    if not rows_mode or ss or n_routed == 0:        # (no read: the gathered form builds the graph of the contigs alone)
        return GATHERED
    return ROWS_BY_PLACE if routes_on_device and not check_rows else ROWS


def k1mer_rows(part, name):
    """the partition's k1-mer file as fixed-width byte rows (kept, or made on demand)"""
    rows = part["k1mer_bytes"][name]
    return rows() if callable(rows) else rows


def with_k1mer_rows(call, part, name, given=None):
    """call(given), and once more with the partition's k1-mer rows where the native stage asks for them: with GPU unitigs it needs
    them only for a partition holding a cycle of condensable edges, built by the sequential code."""
    try:
        return call(given)
    except ShannonError as ex:
        if given is not None or "needs the k1-mer rows" not in str(ex):
            raise
    return call(k1mer_rows(part, name))
