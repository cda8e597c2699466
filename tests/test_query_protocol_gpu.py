"""What the query kinds share, across kinds: the argument rules of every rtbvh_*_async / rtbvh_*_host entry and their
precedence, the isolation of the count blocks, and the ev_query chain under mixed kinds on two streams -- with
growing shared buffers, and with the overflow report of rtbvh_synchronize.  Each kind's answers are pinned to a
brute force by its own test file; here a kind's answer is what it returns when run alone, and every comparison is
bit for bit."""
import ctypes

import numpy as np
import pytest

import raytracebvh_amd as rt
from tests import ray_walk_ref as rw
from tests.conftest import load_scene_fixture

pytestmark = pytest.mark.gpu
W, H = 64, 48
L_ = rt._lib
OK, NOT_READY, INVALID_ARG, OVERFLOW = L_.OK, L_.ERR_NOT_READY, L_.ERR_INVALID_ARG, L_.ERR_STACK_OVERFLOW
K = 4                       # the k of the knn and khits calls
UNKNOWN = 1 << 30           # a mode bit no kind knows
BIG = 1 << 31
SENTINEL = 0xA5             # what the host outputs of a refused call hold, and (PATTERN) the device outputs
PATTERN = 0x5A5AA5A5


class Kind:
    """One pair of entries rtbvh_<name>_async / rtbvh_<name>_host and the Context method over them."""

    def __init__(self, name, inp=None, cols=0, out=None, item=None, k_max=0, bound=False, sort=0, count=4, sizes=0,
                 fill=0, reads=None):
        self.name, self.inp, self.cols = name, inp, cols
        self.out = out              # fixed-size kinds: (float32 or int32 words a record, torch dtype name)
        self.item = item            # list kinds: (words an item, torch dtype name)
        self.k_max, self.bound = k_max, bound
        self.sort, self.count, self.sizes, self.fill = sort, count, sizes, fill
        self.reads = reads or (name,)   # the *_counts readers a counting call of this kind fills
        self.is_list = item is not None
        self.items = {2: "pairs", 4: "hits", 1: "ids"}[item[0]] if item else None   # its lists' word in the messages

    def raw(self, entry, h, inp, n, out, items=None, cap=0, mode=0, stream=None, k=K):
        """The C entry itself.  `out`: the records of a fixed-size kind, the offsets of a list kind."""
        a = [h]
        if self.inp:
            a += [inp, n]
        if self.k_max:
            a.append(k)
        if self.bound:
            a.append(ctypes.c_float(np.inf))
        a.append(out)
        if self.is_list:
            a += [items, cap]
        a.append(mode)
        if entry == "async":
            a.append(stream)
        return getattr(rt.lib(), f"rtbvh_{self.name}_{entry}")(*a)

    def run(self, ctx, inputs, mode=0, capacity=None, stream=None, device=True):
        """Context.<name> of this kind's inputs: a tensor (a tuple of two for a list kind) or numpy arrays."""
        kw = dict(mode=mode)
        if device:
            kw["stream"] = stream
        if self.is_list:
            kw["capacity"] = capacity
        if self.k_max:
            kw["k"] = K
        if not self.inp:
            return ctx.collide(device=device, **kw)
        return getattr(ctx, self.name)(inputs[self.inp], **kw)


KINDS = [
    Kind("query", "rays", 8, out=(4, "float32"), sort=rt.QUERY_SORT, reads=("query", "query_walk")),
    Kind("nearest", "points", 4, out=(8, "float32"), sort=rt.NEAREST_SORT),
    Kind("knn", "points", 4, out=(2 * K, "float32"), k_max=rt.KNN_MAX_K, sort=rt.KNN_SORT),
    Kind("khits", "rays", 8, out=(4 * K, "float32"), k_max=rt.KHITS_MAX_K, sort=rt.KHITS_SORT),
    Kind("signed", "points", 4, out=(8, "float32"), sort=rt.SIGNED_SORT),
    Kind("cross_first", "tris", 12, out=(1, "int32"), sort=rt.CROSS_SORT, reads=("cross",)),
    Kind("clearance", "tris", 12, out=(8, "float32"), bound=True, sort=rt.CLEARANCE_SORT),
    Kind("within", "radius", 4, item=(2, "float32"), sort=rt.WITHIN_SORT, sizes=rt.WITHIN_SIZES, fill=rt.WITHIN_FILL),
    Kind("allhits", "rays", 8, item=(4, "float32"), sort=rt.ALLHITS_SORT, sizes=rt.ALLHITS_SIZES,
         fill=rt.ALLHITS_FILL),
    Kind("overlap", "boxes", 8, item=(1, "int32"), sort=rt.OVERLAP_SORT, sizes=rt.OVERLAP_SIZES,
         fill=rt.OVERLAP_FILL),
    Kind("cross", "tris", 12, item=(1, "int32"), sort=rt.CROSS_SORT, sizes=rt.CROSS_SIZES, fill=rt.CROSS_FILL),
    Kind("region", "regions", 24, item=(1, "int32"), sizes=rt.REGION_SIZES, fill=rt.REGION_FILL),
    Kind("collide", None, 0, item=(1, "int32"), sizes=rt.COLLIDE_SIZES, fill=rt.COLLIDE_FILL),
]
BY_NAME = {k.name: k for k in KINDS}
IDS = [k.name for k in KINDS]
READERS = ["query", "query_walk", "nearest", "knn", "khits", "signed", "cross", "clearance", "within", "allhits",
           "overlap", "region", "region_split", "collide"]


def fixture_scene(name):
    d = load_scene_fixture(name)
    return rt.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])


def context(name, build=True, **kw):
    ctx = rt.Context(device=0, **kw)
    ctx.set_scene(fixture_scene(name))
    ctx.set_camera(*rt.camera_reference(W, H))
    if build:
        ctx.build()
    return ctx


def scene_tris(name):
    s = fixture_scene(name)
    return rw.clip_triangles(s.vertices, s.indices, rt.camera_reference(W, H)[0])


def make_inputs(tris, n, seed):
    """n queries of every input type, inside the scene's box in the space the tree is built in (numpy, packed)."""
    rng = np.random.default_rng(seed)
    flat = tris.reshape(-1, 3)
    lo, hi = flat.min(0), flat.max(0)
    ext = hi - lo

    def inside():
        return (lo + rng.random((n, 3)) * ext).astype(np.float32)

    o, pts, c = inside(), inside(), inside()
    d = inside() - o
    half = ((0.04 + 0.08 * rng.random((n, 1))) * ext).astype(np.float32)
    q = tris[rng.integers(0, len(tris), n)] + (rng.standard_normal((n, 1, 3)) * 0.02 * ext).astype(np.float32)
    r2 = np.float32((0.05 * np.linalg.norm(ext)) ** 2)
    return {"rays": rt.make_rays(o, d), "points": rt.make_points(pts), "radius": rt.make_points(pts, r2),
            "boxes": rt.make_boxes(c - half, c + half), "tris": rt.make_tris(q),
            "regions": rt.box_region(c - half, c + half)}


def on_device(inputs):
    import torch
    cols = {"rays": 8, "points": 4, "radius": 4, "boxes": 8, "tris": 12, "regions": 24}
    dev = {k: torch.from_numpy(v.view(np.float32).reshape(-1, cols[k]).copy()).cuda() for k, v in inputs.items()}
    torch.cuda.synchronize()
    return dev


def host_bytes(res):
    """A result (a tensor, an array, or the (offsets, items) of a list kind) as bytes; a list's items up to its
    total."""
    def arr(x):
        return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    if isinstance(res, tuple):
        off, items = arr(res[0]), arr(res[1])
        return off.tobytes(), np.ascontiguousarray(items[:int(off[-1])]).tobytes()
    return (arr(res).tobytes(),)


def total_of(res):
    return int(res[0][-1].item())


def vp(a):
    return ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


def last_error(ctx):
    return rt.lib().rtbvh_last_error(ctx._h).decode()


# ---------------------------------------------------------------- 1. the argument rules and their precedence
class Buffers:
    """Sentinel-filled inputs and outputs of one kind for both entries: device tensors and numpy arrays."""

    def __init__(self, kind, n=4):
        import torch
        self.kind, self.n = kind, n
        words = kind.item[0] if kind.is_list else kind.out[0]
        self.d_in = torch.zeros((n, max(kind.cols, 1)), dtype=torch.float32, device="cuda")
        self.h_in = np.zeros((n, max(kind.cols, 1)), np.float32)
        rows = 4096 if kind.is_list else n          # (a list kind: room for the items of the one valid call)
        self.d_out = torch.full((rows + 1, words), PATTERN, dtype=torch.int32, device="cuda")
        self.h_out = np.full((rows + 1, words), SENTINEL, np.uint32)
        self.d_off = torch.full((rows + 1,), PATTERN, dtype=torch.int64, device="cuda")   # (collide: T + 1 of them)
        self.h_off = np.full(rows + 1, SENTINEL, np.uint64)
        torch.cuda.synchronize()

    def call(self, entry, ctx, n=None, inp=True, out=True, items=True, cap=8, mode=0, k=K):
        dev = entry == "async"
        i = vp(self.d_in if dev else self.h_in) if inp else None
        n = self.n if n is None else n
        if self.kind.is_list:
            o = vp(self.d_off if dev else self.h_off) if out else None
            it = vp(self.d_out if dev else self.h_out) if items else None
            return self.kind.raw(entry, ctx._h, i, n, o, it, cap, mode, None, k)
        o = vp(self.d_out if dev else self.h_out) if out else None
        return self.kind.raw(entry, ctx._h, i, n, o, mode=mode, k=k)

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return ((self.d_out.cpu().numpy() == PATTERN).all() and (self.d_off.cpu().numpy() == PATTERN).all() and
                (self.h_out == SENTINEL).all() and (self.h_off == SENTINEL).all())


def check_refusals(ctx, kind, entry, state):
    """Every invalid call of one entry, the status of each and -- where two things are wrong -- the message of the
    rule that comes first; then the valid call, refused for `state` ("before build" or "updated")."""
    b = Buffers(kind)
    call = lambda **kw: b.call(entry, ctx, **kw)   # noqa: E731
    has_n = kind.inp is not None
    assert call(mode=UNKNOWN) == INVALID_ARG and "mode bits" in last_error(ctx)
    assert call(mode=UNKNOWN, n=BIG, inp=False, k=0) == INVALID_ARG and "mode bits" in last_error(ctx)
    assert call(mode=UNKNOWN, n=0) == INVALID_ARG and "mode bits" in last_error(ctx)
    if kind.is_list:
        both = kind.sizes | kind.fill
        assert call(mode=both) == INVALID_ARG and "mode bits" in last_error(ctx)
        assert call(mode=both, n=0) == INVALID_ARG and "mode bits" in last_error(ctx)
    if kind.name == "allhits":
        assert call(mode=rt.ALLHITS_SIZES | rt.ALLHITS_BY_T) == INVALID_ARG and "mode bits" in last_error(ctx)
    if kind.name == "region":
        for field in (13, 14):
            assert call(mode=field << rt.REGION_SPLIT_SHIFT, n=BIG) == INVALID_ARG and "split field" in last_error(ctx)
    if kind.k_max:
        for k in (0, kind.k_max + 1):
            for n in (4, 0, BIG):                   # the k rule comes before every rule on n
                assert call(k=k, n=n) == INVALID_ARG and "k must be" in last_error(ctx)
    if has_n:
        assert call(n=BIG) == INVALID_ARG and "2^31" in last_error(ctx)
        assert call(n=BIG, inp=False, out=False) == INVALID_ARG and "2^31" in last_error(ctx)
        assert call(n=0, mode=kind.fill) == OK      # nothing to do, before any look at the pointers or the tree
        assert call(n=0, inp=False, out=False, items=False) == OK
        assert call(inp=False) == INVALID_ARG and "NULL" in last_error(ctx)
    assert call(out=False) == INVALID_ARG and "NULL" in last_error(ctx)
    if kind.is_list:
        assert call(items=False) == INVALID_ARG and "NULL " + kind.items in last_error(ctx)
        assert call(items=False, mode=kind.fill) == INVALID_ARG and "NULL " + kind.items in last_error(ctx)
        assert call(out=False, items=False) == INVALID_ARG and "offsets" in last_error(ctx)   # offsets before items
        if has_n:
            assert call(inp=False, items=False) == INVALID_ARG and "or offsets" in last_error(ctx)
        assert call(items=False, cap=0) == NOT_READY        # no capacity: no list to write to
        assert call(items=False, mode=kind.sizes) == NOT_READY
    assert call() == NOT_READY
    msg = last_error(ctx)
    assert ("before build" in msg) if state == "before build" else ("vertices were updated" in msg), msg
    if kind.sort:
        assert call(mode=kind.sort | kind.count) == NOT_READY
    return b


@pytest.mark.parametrize("entry", ["async", "host"])
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_refusals_and_their_precedence(kind, entry):
    import torch
    with context("Rect", build=False) as ctx:
        b = check_refusals(ctx, kind, entry, "before build")
        # n = 0 of a list kind stores offsets[0] = 0 -- unless the offsets are input (FILL) -- and nothing else
        if kind.is_list and kind.inp:
            assert b.call(entry, ctx, n=0, mode=kind.fill) == OK
            ctx.synchronize()
            assert b.untouched()
            assert b.call(entry, ctx, n=0, mode=kind.count) == OK
            assert b.call(entry, ctx, n=0, mode=kind.sizes, items=False) == OK
            ctx.synchronize()
            torch.cuda.synchronize()
            off = b.d_off.cpu().numpy() if entry == "async" else b.h_off
            rest = PATTERN if entry == "async" else SENTINEL
            assert off[0] == 0 and (off[1:] == rest).all()
            off[0] = rest
            if entry == "async":
                b.d_off.fill_(PATTERN)
        assert b.untouched()
        for name in READERS:
            out = np.zeros(6, np.uint64)
            assert getattr(rt.lib(), f"rtbvh_{name}_counts")(ctx._h, vp(out)) == NOT_READY
            assert getattr(rt.lib(), f"rtbvh_{name}_counts")(ctx._h, None) == INVALID_ARG
    with context("Rect") as ctx:
        d = load_scene_fixture("Rect")
        ctx.update_vertices(d["vertices"][:, :3].copy())
        b = check_refusals(ctx, kind, entry, "updated")
        assert b.untouched()
        ctx.refit()
        assert b.call(entry, ctx, cap=4096) == OK
        ctx.synchronize()
        assert not b.untouched()


# ---------------------------------------------------------------- 2. the count blocks are isolated
CAP = 1 << 16               # the list kinds' capacity: one call each, its counts those of both passes


def read_counts(ctx, reader):
    return getattr(ctx, reader + "_counts")()


def counting_runs():
    """(label, kind, extra mode bits, the readers a counting call fills)."""
    runs = [(k.name, k, 0, k.reads) for k in KINDS]
    runs.append(("region_split", BY_NAME["region"], rt.region_split(4), ("region", "region_split")))
    return runs


def test_count_blocks_are_isolated():
    tris = scene_tris("Test")
    sets = {n: make_inputs(tris, n, seed=n) for n in (64, 48, 32)}
    with context("Test") as ctx:
        seen = {}
        for label, kind, extra, reads in counting_runs():
            for r in reads:
                if r not in seen:                   # no counting query of the kind yet, whatever the others ran
                    with pytest.raises(rt.RtbvhError) as e:
                        read_counts(ctx, r)
                    assert e.value.status == NOT_READY, r
            kind.run(ctx, sets[64], mode=extra, capacity=CAP, device=False)   # (not counting: nothing changes)
            for r in reads:
                if r not in seen:
                    with pytest.raises(rt.RtbvhError):
                        read_counts(ctx, r)
            kind.run(ctx, sets[64], mode=kind.count | extra, capacity=CAP, device=False)
            for r in reads:
                seen[r] = read_counts(ctx, r)
        assert sorted(seen) == sorted(READERS)
        first = {"query": "rays", "nearest": "points", "knn": "points", "khits": "rays", "signed": "points",
                 "cross": "queries", "clearance": "queries", "within": "points", "allhits": "rays",
                 "overlap": "boxes", "region": "regions"}
        for r, field in first.items():
            assert seen[r][field] == 64, r
        assert seen["collide"]["triangles"] == len(tris) and seen["region_split"]["k"] == 4
        assert sum(seen["query_walk"].values()) == 64
        for label, kind, extra, reads in counting_runs():
            kind.run(ctx, sets[48], mode=extra, capacity=CAP, device=False)
            for r in READERS:                       # a query that does not count leaves every block alone
                assert read_counts(ctx, r) == seen[r], (label, r)
            kind.run(ctx, sets[32], mode=kind.count | extra, capacity=CAP, device=False)
            for r in READERS:
                if r not in reads:
                    assert read_counts(ctx, r) == seen[r], (label, r)
            for r in reads:
                seen[r] = read_counts(ctx, r)
                if r in first and kind.inp:
                    assert seen[r][first[r]] == 32, (label, r)


# ---------------------------------------------------------------- 3. mixed kinds on two streams
@pytest.fixture(scope="module")
def alone():
    """A context whose queries run one at a time on the context stream, each behind a synchronize: the answers."""
    ctx = context("Test")
    yield ctx
    ctx.close()


def answer(ctx, kind, dev, mode):
    import torch
    res = kind.run(ctx, dev, mode=mode)             # (torch's default stream: the context stream, synchronized)
    ctx.synchronize()
    torch.cuda.synchronize()
    return res


def test_mixed_kinds_on_two_streams(alone):
    import torch
    dev = on_device(make_inputs(scene_tris("Test"), 512, seed=7))
    want = {k.name: answer(alone, k, dev, k.sort) for k in KINDS}
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with context("Test") as ctx:
        got = {}
        for rounds in range(2):                     # (the second round: every buffer already there)
            for i, k in enumerate(KINDS):
                cap = total_of(want[k.name]) + 16 if k.is_list else None
                got[rounds, k.name] = k.run(ctx, dev, mode=k.sort, capacity=cap, stream=streams[(i + rounds) % 2])
        ctx.synchronize()                           # the one host wait: behind every stream's queries
        for key, res in got.items():
            assert host_bytes(res) == host_bytes(want[key[1]]), key
    for k in KINDS:                                 # the answers say something: lists with members, records with hits
        if k.is_list:
            assert total_of(want[k.name]) > 0, k.name
    assert (want["query"][:, 0] >= 0).any() and (want["cross_first"] >= 0).any()


# ---------------------------------------------------------------- 4. shared buffers that grow mid-chain
def test_buffers_grow_while_the_chain_is_in_flight(alone):
    import torch
    tris = scene_tris("Test")
    small, big = on_device(make_inputs(tris, 64, seed=11)), on_device(make_inputs(tris, 4096, seed=12))
    few = {"regions": big["regions"][:8].contiguous()}
    by_t, auto = rt.ALLHITS_SORT | rt.ALLHITS_BY_T, rt.REGION_SPLIT_AUTO
    calls = [("within", small, rt.WITHIN_SORT), ("allhits", small, by_t),        # the first, small buffers
             ("overlap", big, rt.OVERLAP_SORT),                                  # the sort's and the scan's grow
             ("allhits", big, by_t),                                             # the ordering pass's grow
             ("region", small, rt.region_split(16)), ("region", few, auto),      # the pieces' grow (8 x 4096)
             ("knn", big, rt.KNN_SORT), ("within", small, rt.WITHIN_SORT)]
    want = [answer(alone, BY_NAME[name], dev, mode) for name, dev, mode in calls]
    s = [torch.cuda.Stream(), torch.cuda.Stream()]
    with context("Test") as ctx:
        got = []
        for i, (name, dev, mode) in enumerate(calls):
            kind = BY_NAME[name]
            cap = total_of(want[i]) + 16 if kind.is_list else None
            got.append(kind.run(ctx, dev, mode=mode, capacity=cap, stream=s[i % 2]))
        ctx.synchronize()
        for i, (name, _, mode) in enumerate(calls):
            assert host_bytes(got[i]) == host_bytes(want[i]), (i, name, mode)
    assert total_of(want[3]) > 0                    # lists to order


# ---------------------------------------------------------------- 5. rtbvh_synchronize reports an overflow once
def test_synchronize_reports_the_batch_overflow_once():
    import torch
    dev = on_device(make_inputs(scene_tris("Test"), 256, seed=5))
    s = [torch.cuda.Stream(), torch.cuda.Stream()]
    sync = rt.lib().rtbvh_synchronize
    with context("Test", stack_limit=2) as ctx:
        assert sync(ctx._h) == OK
        for names in (("nearest", "within", "knn", "overlap"), ("nearest",), ("within",)):
            for i, name in enumerate(names):
                kind = BY_NAME[name]
                kind.run(ctx, dev, mode=kind.sort, capacity=64 if kind.is_list else None, stream=s[i % 2])
            assert sync(ctx._h) == OVERFLOW, names  # the walks ran out of stack: reported once ...
            assert sync(ctx._h) == OK, names        # ... and not again until a query overflows anew
