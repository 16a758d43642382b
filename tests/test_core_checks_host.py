"""CPU tier: the argument checks of the eight core entry points and graphop_maskedmm_csr_forward_partial through the
C ABI -- which check answers first, and that a NULL chunked-CSR array is reported under the name the signature gives it.

No call here may reach a kernel launch (the pointers are made up), so this file holds the checks an entry point makes
BEFORE its first zero fill: with sizes that make every fill empty where that is possible.  The NULL-array checks that
stand behind a fill (maskedmm_csr_forward, vector_spmm_forward, the row half of vector_spmm_backward,
node_mul_edge_forward, and the GAT, GATv2 and dot-product attention families but for gat_scores_backward, whose
outputs may all be empty) need real output buffers: they are in
tests/test_core_launches.py, which takes SIGNATURES and call() from here."""
import pytest

SOME = 256          # a pointer that is not NULL and is never dereferenced


def _sig(ptrs, ints, tail):
    return [(n, "p") for n in ptrs.split()] + [(n, "i") for n in ints.split()] + list(tail)


PLAN1 = (("plan", "null"), ("stream", "null"))
PLAN2 = (("plan_r", "null"), ("plan_c", "null"), ("stream", "null"))
WS = (("workspace", "p"), ("workspace_bytes", "i"))
WS_ROWS = (("workspace", "p"), ("workspace_rows", "i"))
SLOPE = (("negative_slope", "f"),)
# entry point -> its arguments after dtype, in the order of include/graphop_hip.h: (name, kind)
SIGNATURES = {
    "maskedmm_csr_forward": _sig("row indptr eid indices A B y", "n_chunks n_edges n_a n_b h d", PLAN1),
    "maskedmm_csr_forward_partial": _sig("row indptr eid indices A B y", "n_chunks n_slots n_y n_a n_b h d",
                                         (("stream", "null"),)),
    "maskedmm_csr_backward": _sig("row indptr_r eid_r indices_r col indptr_c eid_c indices_c A B dy dA dB",
                                  "n_row_chunks n_col_chunks n_edges n_a n_b h d", PLAN2),
    "sparse_softmax_forward": _sig("row indptr eid x y", "n_chunks n_edges h", WS_ROWS + PLAN1),
    "sparse_softmax_backward": _sig("row indptr eid y dy dx", "n_chunks n_edges h", WS_ROWS + PLAN1),
    "vector_spmm_forward": _sig("row indptr eid indices edata x y", "n_chunks n_edges n_x n_y h d", PLAN1),
    "vector_spmm_backward": _sig("row indptr eid indices col indptr_t eid_t indices_t edata dy x dedata dx",
                                 "n_row_chunks n_col_chunks n_edges n_x n_dy h d", PLAN2),
    "node_mul_edge_forward": _sig("row indptr eid A B y", "n_chunks n_edges n_a h d", PLAN1),
    "node_mul_edge_backward": _sig("row indptr eid A B dy dA dB", "n_chunks n_edges n_a h d", PLAN1),
    # one forward and one backward of each family of extra ops
    "gat_scores_forward": _sig("row indptr eid indices el er y", "n_chunks n_edges n_l n_r h", SLOPE + PLAN1),
    "gat_scores_backward": _sig("row indptr_r eid_r indices_r col indptr_c eid_c indices_c el er dy del der",
                                "n_row_chunks n_col_chunks n_edges n_l n_r h", SLOPE + PLAN2),
    "gatv2_scores_forward": _sig("row indptr eid indices xl xr att y", "n_chunks n_edges n_l n_r h d", SLOPE + PLAN1),
    "gatv2_scores_backward": _sig("row indptr_r eid_r indices_r col indptr_c eid_c indices_c xl xr att dy dxl dxr datt "
                                  "workspace", "workspace_bytes n_row_chunks n_col_chunks n_edges n_l n_r h d",
                                  SLOPE + PLAN2),
    "attention_forward": _sig("row indptr eid indices Q K V o stats", "n_chunks n_edges n_q n_k h d", WS + PLAN1),
    "attention_backward": _sig("row indptr_r eid_r indices_r col indptr_c eid_c indices_c Q K V o stats dO dQ dK dV",
                               "n_row_chunks n_col_chunks n_edges n_q n_k h d", WS + PLAN2),
}
CORE = list(SIGNATURES)[:9]
CSR_NAMES = {"row", "indptr", "eid", "indices", "col", "indptr_r", "eid_r", "indices_r", "indptr_c", "eid_c", "indices_c",
             "indptr_t", "eid_t", "indices_t"}


def csr_arrays(name):
    return [n for n, kind in SIGNATURES[name] if kind == "p" and n in CSR_NAMES]


def call(l, name, dtype=0, null=(), ptr=SOME, ws_bytes=0, **sizes):
    """the entry point with every pointer = ptr (a dict: ptr[name], else ptr[None]) except those named in `null`
    (null="all": every one), every size the one given (sizes not named: 1); -> (return code, message)"""
    args = [dtype]
    for n, kind in SIGNATURES[name]:
        if kind == "p":
            args.append(None if null == "all" or n in null else ptr.get(n, ptr[None]) if isinstance(ptr, dict) else ptr)
        elif kind == "i":
            args.append(ws_bytes if n == "workspace_bytes" else sizes.pop(n, 1))
        elif kind == "f":
            args.append(0.2)
        else:
            args.append(None)
    assert not sizes, sizes
    rc = getattr(l, "graphop_" + name)(*args)
    return rc, l.graphop_last_error() if rc else b""


@pytest.fixture(scope="module")
def l():
    from custom_op_benchmark_amd import _lib
    return _lib.lib()


# entry point -> [(the arrays checked, the sizes under which their check comes before any zero fill)]
BEFORE_ANY_FILL = {
    "maskedmm_csr_forward_partial": [(("row", "indptr", "eid", "indices"),
                                      dict(n_chunks=4, n_slots=10, n_y=10, n_a=5, n_b=5, d=8))],
    "maskedmm_csr_backward": [(("row", "indptr_r", "eid_r", "indices_r"),
                               dict(n_row_chunks=4, n_col_chunks=0, n_edges=10, n_a=0, n_b=0, d=8)),
                              (("col", "indptr_c", "eid_c", "indices_c"),
                               dict(n_row_chunks=0, n_col_chunks=4, n_edges=10, n_a=0, n_b=0, d=8))],
    "sparse_softmax_forward": [(("row", "indptr", "eid"), dict(n_chunks=4, n_edges=10, h=2))],
    "sparse_softmax_backward": [(("row", "indptr", "eid"), dict(n_chunks=4, n_edges=10, h=2))],
    "vector_spmm_backward": [(("col", "indptr_t", "eid_t", "indices_t"),
                              dict(n_row_chunks=4, n_col_chunks=4, n_edges=0, n_x=0, n_dy=5, d=8))],
    "node_mul_edge_backward": [(("row", "indptr", "eid"), dict(n_chunks=4, n_edges=0, n_a=0, d=8))],
    # of the families, the one op whose outputs can all be empty while its passes still run
    "gat_scores_backward": [(("row", "indptr_r", "eid_r", "indices_r"),
                             dict(n_row_chunks=4, n_col_chunks=0, n_edges=10, n_l=0, n_r=0)),
                            (("col", "indptr_c", "eid_c", "indices_c"),
                             dict(n_row_chunks=0, n_col_chunks=4, n_edges=10, n_l=0, n_r=0))],
}
# sizes under which the parent accepts every pointer NULL without a launch
EMPTY_OK = {
    "maskedmm_csr_forward": [dict(n_chunks=4, n_edges=0, n_a=5, n_b=5, d=8), dict(n_chunks=0, n_edges=0)],
    "maskedmm_csr_forward_partial": [dict(n_chunks=0, n_slots=10, n_y=10, n_a=5, n_b=5, d=8),
                                     dict(n_chunks=4, n_slots=0, n_y=0, d=8)],
    "maskedmm_csr_backward": [dict(n_row_chunks=0, n_col_chunks=0, n_edges=10, n_a=0, n_b=0, d=8),
                              dict(n_row_chunks=4, n_col_chunks=4, n_edges=10, n_a=0, n_b=0, d=0)],
    "sparse_softmax_forward": [dict(n_chunks=4, n_edges=0), dict(n_chunks=0, n_edges=0)],
    "sparse_softmax_backward": [dict(n_chunks=4, n_edges=0), dict(n_chunks=0, n_edges=0)],
    "vector_spmm_forward": [dict(n_chunks=4, n_edges=10, n_x=5, n_y=0, d=8), dict(n_chunks=0, n_edges=0, n_y=5, d=0)],
    "vector_spmm_backward": [dict(n_row_chunks=0, n_col_chunks=0, n_edges=0, n_x=0, n_dy=5, d=8),
                             dict(n_row_chunks=4, n_col_chunks=0, n_edges=0, n_x=0, n_dy=5, d=8)],
    "node_mul_edge_forward": [dict(n_chunks=4, n_edges=0, n_a=5, d=8), dict(n_chunks=0, n_edges=0)],
    "node_mul_edge_backward": [dict(n_chunks=0, n_edges=0, n_a=0, d=8), dict(n_chunks=4, n_edges=0, n_a=0, d=0)],
}


def test_the_tables_cover_the_nine_entry_points():
    assert len(CORE) == 9 and set(EMPTY_OK) == set(CORE) and set(BEFORE_ANY_FILL) <= set(SIGNATURES)
    from custom_op_benchmark_amd import _lib
    for name, sig in SIGNATURES.items():
        assert len(sig) + 1 == len(_lib._SIGNATURES["graphop_" + name]), name
    for name, cases in BEFORE_ANY_FILL.items():
        for arrays, _ in cases:
            assert set(arrays) <= set(csr_arrays(name)), name


@pytest.mark.parametrize("name", sorted(BEFORE_ANY_FILL))
def test_a_null_csr_array_is_named_as_in_the_signature(l, name):
    for arrays, sizes in BEFORE_ANY_FILL[name]:
        for a in arrays:
            rc, msg = call(l, name, null=(a,), **sizes)
            assert rc == 1 and msg == ("%s: %s is NULL" % (name, a)).encode(), (name, a, rc, msg)
        # ... and the arrays are asked for in the signature's order
        rc, msg = call(l, name, null=arrays, **sizes)
        assert rc == 1 and msg == ("%s: %s is NULL" % (name, arrays[0])).encode(), (name, rc, msg)


@pytest.mark.parametrize("name", CORE)
def test_empty_problems_accept_null_arrays(l, name):
    for sizes in EMPTY_OK[name]:
        assert call(l, name, null="all", **sizes) == (0, b""), (name, sizes)
        assert call(l, name, dtype=1, null="all", **sizes) == (0, b""), (name, sizes)


@pytest.mark.parametrize("name", list(SIGNATURES))
def test_negative_sizes_and_the_dtype_come_first(l, name):
    counts = [n for n, kind in SIGNATURES[name] if kind == "i" and (n.endswith("chunks") or n in ("n_edges", "n_slots"))]
    for n in counts[:1] + counts[-1:]:
        rc, msg = call(l, name, null="all", **{n: -1})
        assert rc == 1 and msg.startswith(name.encode() + b": ") and b"negative size" in msg, (name, n, rc, msg)
    # a bad dtype is reported before a NULL array (non-zero counts, every pointer NULL) and before a negative size
    big = {n: 4 for n, kind in SIGNATURES[name] if kind == "i" and n != "workspace_bytes"}
    for sizes in (big, {**big, counts[0]: -1}):
        rc, msg = call(l, name, dtype=7, null="all", **sizes)
        want = b": bad dtype" if name.startswith("attention") else b": dtype must be GRAPHOP_F32 or GRAPHOP_F64"
        assert rc == 1 and msg == name.encode() + want, (name, rc, msg)


def test_partial_sddmm_size_rule(l):
    rc, msg = call(l, "maskedmm_csr_forward_partial", null="all", n_chunks=4, n_slots=10, n_y=9, d=8)
    assert rc == 1 and b"n_y (9) must be at least n_slots (10)" in msg
    rc, msg = call(l, "maskedmm_csr_forward_partial", null=("y",), n_chunks=4, n_slots=10, n_y=10, n_a=5, n_b=5, d=8)
    assert rc == 1 and msg == b"maskedmm_csr_forward_partial: y is NULL"


def test_outputs_are_asked_for_before_the_arrays(l):
    """the output that would be zero-filled first is the first NULL reported"""
    for name, out, sizes in (("maskedmm_csr_forward", "y", dict(n_chunks=4, n_edges=10, n_a=5, n_b=5, d=8)),
                             ("sparse_softmax_forward", "y", dict(n_chunks=4, n_edges=10)),
                             ("sparse_softmax_backward", "dx", dict(n_chunks=4, n_edges=10)),
                             ("vector_spmm_forward", "y", dict(n_chunks=4, n_edges=10, n_x=5, n_y=5, d=8)),
                             ("vector_spmm_backward", "dedata",
                              dict(n_row_chunks=4, n_col_chunks=4, n_edges=10, n_x=5, n_dy=5, d=8)),
                             ("maskedmm_csr_backward", "dA",
                              dict(n_row_chunks=4, n_col_chunks=4, n_edges=10, n_a=5, n_b=5, d=8)),
                             ("node_mul_edge_forward", "y", dict(n_chunks=4, n_edges=10, n_a=5, d=8)),
                             ("node_mul_edge_backward", "dA", dict(n_chunks=4, n_edges=10, n_a=5, d=8))):
        rc, msg = call(l, name, null="all", **sizes)
        assert rc == 1 and msg == ("%s: %s is NULL" % (name, out)).encode(), (name, rc, msg)
