"""A guard around everything the ctypes binding allocates: outputs, workspaces and plan memory sit between
bands of GUARD poisoned bytes, float outputs start as NaN, float operands sit between NaN bands.  After a call the bands
must still hold their poison (no store outside a block), a returned output holds no NaN (no element left unwritten; a
stray operand read shows as a NaN too) and the inputs are bitwise what they were.

Imports without a GPU: tests/test_guarded_host.py runs the harness on CPU tensors, tests/test_guarded.py on the device.

What the guard cannot see: an access more than GUARD bytes away from its block, a stray read of an index array (no bands:
it would be used as an address), the C++ bindings (they allocate in C++), captured graphs and the RCCL exchange buffers."""
import contextlib
import functools
import gc

import torch

GUARD = 4096          # bytes on either side: a multiple of 512, so a view keeps the alignment class of a torch.empty block
POISON = 0xA5
SPELLINGS = ("empty", "empty_like", "zeros", "zeros_like")          # what graphop.py allocates with


def _shape_of(size):
    if len(size) == 1 and not isinstance(size[0], int):
        return tuple(int(n) for n in size[0])
    return tuple(int(n) for n in size)


class GuardedTorch:
    """Stand-in for the module global `torch` of custom_op_benchmark_amd/graphop.py: empty, empty_like, zeros and zeros_like
    return a contiguous view inside a uint8 buffer of nbytes + 2 * GUARD filled with POISON; an empty* view of a floating
    dtype is filled with NaN (another dtype keeps the poison), a zeros* view is zeroed.  Everything else is torch's."""

    def __init__(self):
        self.records = []          # (buffer, nbytes, view, kind) per allocation, in order

    def __getattr__(self, name):
        return getattr(torch, name)

    def _alloc(self, shape, dtype, device, kind):
        dtype = dtype if dtype is not None else torch.get_default_dtype()
        numel = 1
        for n in shape:
            numel *= n
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        buf = torch.empty(nbytes + 2 * GUARD, dtype=torch.uint8, device=device)
        buf.fill_(POISON)
        view = buf[GUARD:GUARD + nbytes].view(dtype).view(shape)
        if kind.startswith("zeros"):
            view.zero_()
        elif dtype.is_floating_point:
            view.fill_(float("nan"))
        self.records.append((buf, nbytes, view, kind))
        return view

    def empty(self, *size, dtype=None, device=None):
        return self._alloc(_shape_of(size), dtype, device, "empty")

    def zeros(self, *size, dtype=None, device=None):
        return self._alloc(_shape_of(size), dtype, device, "zeros")

    def empty_like(self, t):
        return self._alloc(tuple(t.shape), t.dtype, t.device, "empty_like")

    def zeros_like(self, t):
        return self._alloc(tuple(t.shape), t.dtype, t.device, "zeros_like")

    # ---- the checks ------------------------------------------------------------------------------------------------
    def guarded_bytes(self):
        return sum(r[1] for r in self.records)

    def violations(self, outputs=()):
        """[str]: every band byte that is not POISON, with the allocation's index, shape, side and byte offset (before: from
        the view's first byte, negative; after: from the first byte past it), and every NaN left in an empty* float view
        that is one of `outputs` (tensors, or nested lists / dicts of them; matched by storage, so a detached or reshaped
        result counts).  Workspaces -- allocations not among `outputs` -- are exempt from the NaN rule only."""
        if torch.cuda.is_available() and any(r[0].is_cuda for r in self.records):
            torch.cuda.synchronize()
        out = []
        returned = {t.untyped_storage().data_ptr() for t in _flatten(outputs) if t.numel() > 0}
        if self.records:
            # one pass that only counts, so a clean run costs one read-back per device
            dirty = torch.stack([(buf[:GUARD] != POISON).sum() + (buf[GUARD + n:] != POISON).sum()
                                 for buf, n, _, _ in self.records]).cpu().tolist()
        for i, (buf, n, view, kind) in enumerate(self.records):
            if dirty[i]:
                for side, band, origin in (("before", buf[:GUARD], -GUARD), ("after", buf[GUARD + n:], 0)):
                    bad = (band != POISON).nonzero().flatten().cpu().tolist()
                    if bad:
                        out.append("allocation %d (%s %s %s): %d byte(s) of the band %s it overwritten, first at byte offset "
                                   "%d, last at %d" % (i, kind, tuple(view.shape), view.dtype, len(bad), side,
                                                       origin + bad[0], origin + bad[-1]))
            if kind.startswith("empty") and view.dtype.is_floating_point and n and \
                    buf.untyped_storage().data_ptr() in returned:
                nan = torch.isnan(view).reshape(-1)
                if bool(nan.any()):
                    first = int(nan.nonzero()[0])
                    out.append("allocation %d (%s %s %s): %d element(s) of a returned output never written, first at flat "
                               "index %d" % (i, kind, tuple(view.shape), view.dtype, int(nan.sum()), first))
        return out


def _flatten(x):
    if isinstance(x, torch.Tensor):
        yield x
    elif isinstance(x, dict):
        for v in x.values():
            yield from _flatten(v)
    elif isinstance(x, (list, tuple, set)):
        for v in x:
            yield from _flatten(v)


@contextlib.contextmanager
def guarded_ops():
    """Installs a GuardedTorch as graphop.torch and restores the module on exit, also after an exception.
    -> the GuardedTorch: .violations(outputs) synchronises and reports, .records / .guarded_bytes() count."""
    from custom_op_benchmark_amd import graphop
    real, g = graphop.torch, GuardedTorch()
    graphop.torch = g
    try:
        yield g
    finally:
        graphop.torch = real


def banded(t, device=None):
    """A copy of the float tensor t (on `device`, if given) as a view between NaN bands of GUARD bytes, at the alignment of
    a torch.empty block: a stray read next to the operand is a NaN in a result instead of nothing.  Index arrays get no
    bands (and come back as they are, moved to `device`)."""
    device = t.device if device is None else device
    if not t.dtype.is_floating_point:
        return t.to(device)
    pad = GUARD // t.element_size()
    buf = torch.full((t.numel() + 2 * pad,), float("nan"), dtype=t.dtype, device=device)
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).clone()


def snapshot(tensors):
    """[(tensor, its bytes now)] of every tensor in `tensors` (nested lists / dicts too)"""
    return [(t, _bits(t)) for t in _flatten(tensors)]


def unchanged(snap):
    """[str]: every tensor of the snapshot whose bytes differ now -- compared as integers, so NaN payloads count"""
    out = []
    for i, (t, was) in enumerate(snap):
        diff = (_bits(t) != was).nonzero().flatten()
        if diff.numel():
            out.append("input %d %s %s: %d byte(s) changed, first at byte offset %d"
                       % (i, tuple(t.shape), t.dtype, diff.numel(), int(diff[0])))
    return out


# ---- plan memory ---------------------------------------------------------------------------------------------------------------
_blocks = {}          # pointer handed to the library -> (block with its bands, bytes asked)
_damage = []          # what the free callback found: a callback cannot raise through C
_counts = {"blocks": 0, "bytes": 0}


def _alloc_cb(nbytes, device, stream):
    # as _lib._alloc_cb: on the stream the library names; the whole block, interior included, is POISON
    try:
        dev = torch.device("cuda", device)
        n = max(1, int(nbytes))
        ctx = torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=dev)) if stream else contextlib.nullcontext()
        with ctx:
            t = torch.empty(n + 2 * GUARD, dtype=torch.uint8, device=dev)
            t.fill_(POISON)
    except RuntimeError:
        return None
    p = t.data_ptr() + GUARD
    _blocks[p] = (t, n)
    _counts["blocks"] += 1
    _counts["bytes"] += n
    return p


def _free_cb(p):
    from custom_op_benchmark_amd import _lib
    ent = _blocks.pop(p, None)
    if ent is None:               # a block from before the guard was installed
        _lib._free_cb(p)
        return
    try:
        t, n = ent
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.synchronize(t.device)
            _damage.extend(_band_damage(t, n))
    except Exception as e:        # (never through C)
        _damage.append("free callback: %r" % (e,))


def _band_damage(t, n):
    out = []
    if not int(((t[:GUARD] != POISON).sum() + (t[GUARD + n:] != POISON).sum()).item()):
        return out
    for side, band, origin in (("before", t[:GUARD], -GUARD), ("after", t[GUARD + n:], 0)):
        bad = (band != POISON).nonzero().flatten().cpu().tolist()
        if bad:
            out.append("plan block of %d bytes: %d byte(s) of the band %s it overwritten, first at byte offset %d, last at %d"
                       % (n, len(bad), side, origin + bad[0], origin + bad[-1]))
    return out


_CALLBACKS = None     # the ctypes callback objects, kept alive for the life of the module


@contextlib.contextmanager
def guarded_plan_memory():
    """Plan memory between poisoned bands: clears the plan cache, registers an alloc / free pair of its own through
    graphop_set_allocator, and on exit clears the cache again -- every guarded block is freed through the guarded pair, which
    checks its bands -- and re-registers the binding's own pair.  -> the list the free callback appends damage to: the
    caller asserts it is empty AFTER the with block.  A plan the caller still holds at exit outlives the guard: that is
    reported as damage too (its block goes on to the binding's pair, unchecked)."""
    global _CALLBACKS
    from custom_op_benchmark_amd import _lib
    lib = _lib.lib()
    if _CALLBACKS is None:
        _CALLBACKS = (_lib.ALLOC_FN(_alloc_cb), _lib.FREE_FN(_free_cb))
    _lib.clear_plan_cache()
    gc.collect()
    del _damage[:]
    _lib.check(lib.graphop_set_allocator(*_CALLBACKS))
    try:
        yield _damage
    finally:
        _lib.clear_plan_cache()
        gc.collect()
        for p, (t, n) in list(_blocks.items()):
            _damage.append("plan block of %d bytes is still held at the end of the guard" % n)
            _lib._live_blocks[p] = t          # freed later through the binding's own callback
            del _blocks[p]
        _lib.check(lib.graphop_set_allocator(_lib._ALLOC_CB, _lib._FREE_CB))


def plan_memory_counts():
    """(blocks, bytes) the guarded plan allocator has handed out in this process"""
    return _counts["blocks"], _counts["bytes"]


# ---- the cases of tests/test_guarded.py: graphs and draws, computed without a GPU -------------------------------------------
def ctypes_entry(case):
    """a battery's case through the ctypes entry with a contiguous output gradient, as tests/test_attention_fuzz.py takes
    a case for its launch profile: the C++ bindings allocate in C++, out of the guard's reach"""
    import dataclasses
    return dataclasses.replace(case, entry="ctypes", grad_view="contiguous")


@functools.lru_cache(maxsize=None)
def core_fuzz_graph(seed):
    """the graph test_hip_parity.test_fuzz_shapes_and_paths builds for a seed"""
    from test_hip_parity import fuzz_case
    from util import random_graph
    shape, _, _ = fuzz_case(seed)
    n_src, n_dst, n_edges, cs, hub = (shape[x] for x in ("n_src", "n_dst", "n_edges", "cs", "hub"))
    g = random_graph(n_src, n_dst, n_edges, seed=seed, chunk_size=cs, zero_rows=shape["zero_rows"], hub=hub or None)
    if g.n_dst < g.n_src:          # the reference's SpMM output is zeros_like(x): x (n_dst rows) must cover the row ids
        g = random_graph(n_src, n_src, n_edges, seed=seed, chunk_size=cs, hub=hub or None)
    return g


def fp64_graph(d):
    """test_hip_parity.test_step_vs_oracle_fp64"""
    from util import random_graph
    return random_graph(120, 150, 2000, seed=d, chunk_size=8, zero_rows=0.1, hub=300)


def walk_graph():
    """test_walk.test_fp64_on_the_walk_and_window_drivers_vs_oracle at d = 32, walk_blocks = 8"""
    from util import random_graph
    return random_graph(1500, 1541, 15000, seed=5 + 32 + 8, chunk_size=32, zero_rows=0.15, hub=900)


def shuffled_graph():
    """(g, the eight index arrays with both chunk lists shuffled) of test_hip_parity.test_unordered_chunks_take_the_general_path"""
    from util import random_graph
    g = random_graph(150, 150, 5000, seed=11, chunk_size=8, hub=300)
    gen = torch.Generator().manual_seed(0)

    def shuffled(row, ptr):
        perm = torch.randperm(row.numel(), generator=gen)
        lens = (ptr[1:] - ptr[:-1])[perm]
        new_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
        slot = torch.cat([torch.arange(int(ptr[c]), int(ptr[c + 1])) for c in perm.tolist()])
        return row[perm].contiguous(), new_ptr, slot

    row, ptr_r, sr = shuffled(g.row, g.ptr_r)
    col, ptr_c, sc = shuffled(g.col, g.ptr_c)
    return g, (row, ptr_r, g.eid_r[sr].contiguous(), g.indices_r[sr].contiguous(),
               col, ptr_c, g.eid_c[sc].contiguous(), g.indices_c[sc].contiguous())


def softmax_hub_graph(h):
    """test_hip_parity.test_softmax_long_rows_and_cached_rows"""
    from util import random_graph
    return random_graph(400, 400, 30000, seed=5 + h, chunk_size=32, zero_rows=0.1, hub=20000)


def softmax_lengths_graph(h):
    """(g, the generator after it) of test_hip_parity.test_softmax_several_heads_float4_items"""
    from custom_op_benchmark_amd import graphs
    gen = torch.Generator().manual_seed(40 + h)
    lens = torch.cat([torch.randint(0, 40, (300,), generator=gen), torch.randint(250, 400, (20,), generator=gen),
                      torch.randint(700, 1024, (12,), generator=gen), torch.tensor([1025, 2000, 5000, 0, 1, 1024])])
    lens = lens[torch.randperm(len(lens), generator=gen)]
    n = len(lens)
    src = torch.repeat_interleave(torch.arange(n), lens)
    dst = torch.randint(0, n, (int(lens.sum()),), generator=gen)
    return graphs.graph_from_coo(src, dst, n, n, chunk_size=32), gen


@functools.lru_cache(maxsize=None)
def outside_graph():
    """the graph of the ops outside the batteries: 260 rows by 190 neighbours, chunks of 8, empty rows, a hub row; 4,566
    edges -- E % 4 == 2, so every (E, h) fp32 tensor with odd h and dxe at (3, 5) end off a 16-byte boundary"""
    from util import random_graph
    return random_graph(260, 190, 5000, seed=11, chunk_size=8, zero_rows=0.2, hub=500)


NODE_MUL_EDGE_HD = ((1, 64), (8, 64), (2, 5), (3, 64))
WEIGHTS_H = (1, 4, 8, 3)
EDGE_OUTPUTS = ("s", "a", "dedata", "y", "db", "dxe", "dee", "weights a")


def edge_outputs(n_cu=256):
    """[(output name, case, dtype name, bytes)] of every edge-sized output the guarded cases of the small strata return
    (the large stratum's graphs are sized by the device), and [(family, case)] of the fp64 cases: from the draws alone"""
    import attention_fuzz as AF
    import gat_edge_fuzz as GEF
    import gat_fuzz as GF
    from test_hip_parity import fuzz_case
    sizes, fp64 = [], []
    size = {"float32": 4, "float64": 8}
    for seed in range(48):
        shape, _, _ = fuzz_case(seed)
        e = core_fuzz_graph(seed).n_edges
        for name in ("s", "a", "dedata"):
            sizes.append((name, "core %d" % seed, "float32", e * shape["h"] * 4))
    fp64 += [("core", "fp64 %d x %d" % hd) for hd in ((1, 64), (4, 16), (3, 5))] + [("core", "fp64 walk")]
    for seed in range(GF.N_SUITE):
        case = GF.draw(seed)
        if case.dtype == "float64":
            fp64.append((case.family, "gat %d" % seed))
        if not case.large and case.family in ("gat_scores", "gatv2_scores"):
            e = GF.drawn_graph(case, n_cu).n_edges
            sizes.append(("y", "gat %d" % seed, case.dtype, e * case.h * size[case.dtype]))
    for seed in range(GEF.N_SUITE):
        case = GEF.draw(seed)
        if case.dtype == "float64":
            fp64.append((case.family, "gat_edge %d" % seed))
        if not case.large and case.need_dee:
            e = GF.drawn_graph(case, n_cu).n_edges
            sizes.append(("dee", "gat_edge %d" % seed, case.dtype, e * case.h * size[case.dtype]))
    for seed in range(AF.N_SUITE):
        case = AF.draw(seed)
        if case.dtype == "float64":
            fp64.append((case.family, "attention %d" % seed))
        if case.large:
            continue
        e = AF.drawn_graph(case, n_cu).n_edges
        if case.family == "weights":
            sizes.append(("weights a", "attention %d" % seed, case.dtype, e * case.h * size[case.dtype]))
        if case.op == "bias" and case.need_dx and case.dO:
            sizes.append(("db", "attention %d" % seed, case.dtype, e * case.h * size[case.dtype]))
        if case.op == "edge" and case.need_dx and case.dO:
            sizes.append(("dxe", "attention %d" % seed, case.dtype, e * case.h * case.d * size[case.dtype]))
    e = outside_graph().n_edges          # the hand cases
    sizes += [("y", "node_mul_edge %d x %d" % hd, "float32", e * hd[0] * 4) for hd in NODE_MUL_EDGE_HD]
    sizes += [("weights a", "gat weights h=%d" % h, "float32", e * h * 4) for h in WEIGHTS_H]
    sizes.append(("dxe", "attention_edge 3 x 5", "float32", e * 15 * 4))
    return sizes, fp64
