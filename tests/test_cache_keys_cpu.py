"""Host-only: what the library remembers between calls, and when it notices that the source changed.

Three caches are pure host code and are driven here with CPU tensors:
  ops._cached_weight_op      packed / transformed weights, a global dict of at most ops._WEIGHT_CACHE_MAX entries keyed on
                             id(base) + a weak reference, the view geometry, the layout tag and (base.data_ptr(), base._version);
                             `build` is a counting callable here, so a hit and a miss are exact observations
  render._topology           vertex -> corner CSR and int32 faces, an attribute (_gif_csr) on the faces tensor
  antialias.edge_adjacency   edge adjacency, an attribute (_gif_edge_adj) on the faces tensor
The faces caches are compared with the tables of a fresh faces.clone() (no attribute: built from the current contents).

One caller duty is documented and NOT asserted: a write through `.data` into the same storage bumps no version counter and moves no
address; the caller announces it (ops.clear_weight_cache(); `del faces._gif_csr` / `del faces._gif_edge_adj`).  The test of that
contract asserts only that the announced form rebuilds.
"""
import copy
import gc
import weakref

import numpy as np
import pytest
import torch

from gif_amd import antialias, ops, render


class Build:
    """A counting `build`: every call returns a new object that names the call."""

    def __init__(self, name="b"):
        self.name, self.n = name, 0

    def __call__(self):
        self.n += 1
        return (self.name, self.n)


@pytest.fixture(autouse=True)
def clean_cache(monkeypatch):
    monkeypatch.setattr(ops, "WEIGHT_CACHE", True)
    ops.clear_weight_cache()
    yield
    ops.clear_weight_cache()


def _w(seed=0, shape=(6, 4, 3, 3)):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


TAG = ("pack", True, 8, 4, 1.0, torch.float32, "f32", False)


# ----------------------------------------------------------------------------------------------------------------- weight cache
def test_repeated_call_hits():
    w, b = _w(), Build()
    first = ops._cached_weight_op(w, TAG, b)
    again = ops._cached_weight_op(w, TAG, b)
    assert b.n == 1 and again is first
    assert len(ops._weight_cache) == 1
    # a view of the whole tensor made anew each call (what `weight[0]`-style indexing in a layer gives) hits its own entry too
    v1 = ops._cached_weight_op(w[1:3], TAG, b)
    v2 = ops._cached_weight_op(w[1:3], TAG, b)
    assert b.n == 2 and v2 is v1


def test_distinct_entries_for_one_base():
    """tags (forward / data gradient, wscale, form), two equal-shape slices at different offsets, a permuted-stride view: one entry
    each, every one a hit on its second call and none answering for another"""
    base = _w(1, (8, 4, 3, 3))
    fwd = ("pack", True, 8, 4, 1.0, torch.float32, "f32", False)
    cases = {
        "fwd": (base, fwd),
        "dgrad": (base, ("pack", False, 4, 8, 1.0, torch.float32, "f32", False)),
        "wscale": (base, ("pack", True, 8, 4, 0.5, torch.float32, "f32", False)),
        "form_x3": (base, ("pack", True, 8, 4, 1.0, torch.float32, "f32x3", False)),
        "form_h2x3": (base, ("pack", True, 8, 4, 1.0, torch.float32, "f32h2x3", False)),
        "form_f16": (base, ("pack", True, 8, 4, 1.0, torch.float16, "f16", False)),
        "tapdense": (base, ("pack", True, 8, 4, 1.0, torch.float32, "f32x3", True)),
        "wino": (base, ("wino", True, 8, 4, 1.0, "native")),
        "wino_x3": (base, ("wino", True, 8, 4, 1.0, "bf16x3")),
        "wsq": (base, ("wsq",)),
        "slice_lo": (base[0:4], fwd),
        "slice_hi": (base[4:8], fwd),
        "permuted": (base.permute(0, 1, 3, 2), fwd),
    }
    assert base[0:4].shape == base[4:8].shape and base.permute(0, 1, 3, 2).shape == base.shape
    builds = {k: Build(k) for k in cases}
    first = {k: ops._cached_weight_op(v, tag, builds[k]) for k, (v, tag) in cases.items()}
    assert len(ops._weight_cache) == len(cases)
    for k, (v, tag) in cases.items():
        assert ops._cached_weight_op(v, tag, builds[k]) is first[k], k
    assert {k: b.n for k, b in builds.items()} == {k: 1 for k in cases}
    assert sorted(first.values()) == sorted((k, 1) for k in cases)


def _adam(foreach):
    def change(w, new):
        w.grad = torch.ones_like(w)
        torch.optim.Adam([w], lr=0.1, foreach=foreach).step()
    return change


def _load_state_dict(w, new):
    m = torch.nn.Module()
    m.weight = w
    m.load_state_dict({"weight": new})


def _no_grad_inplace(w, new):
    with torch.no_grad():
        w.mul_(0.5)


def _copy(w, new):
    with torch.no_grad():
        w.copy_(new)


def _slice_write(w, new):
    with torch.no_grad():
        w[1:2] = new[1:2]


def _detach_write(w, new):
    w.detach().add_(1.0)


def _increment_version(w, new):
    torch.autograd.graph.increment_version(w)


def _data_swap(w, new):
    w.data = new


CHANGES = {"no_grad_inplace": _no_grad_inplace, "copy_": _copy, "slice_write": _slice_write, "detach_write": _detach_write,
           "adam_foreach": _adam(True), "adam_single": _adam(False), "load_state_dict": _load_state_dict,
           "increment_version": _increment_version, "data_swap": _data_swap}


@pytest.mark.parametrize("how", list(CHANGES))
@pytest.mark.parametrize("view", ["whole", "slice"])
def test_miss_after_the_source_changes(how, view):
    """every way a parameter's contents (or storage) change makes the next call build, for the tensor itself and for a view of it;
    after that the new entry hits again"""
    w = torch.nn.Parameter(_w(2))
    arg = (lambda: w) if view == "whole" else (lambda: w[2:5])
    b = Build()
    first = ops._cached_weight_op(arg(), TAG, b)
    assert ops._cached_weight_op(arg(), TAG, b) is first and b.n == 1
    CHANGES[how](w, _w(3))
    second = ops._cached_weight_op(arg(), TAG, b)
    assert b.n == 2 and second == ("b", 2), f"{how}: a stale entry answered"
    assert ops._cached_weight_op(arg(), TAG, b) is second and b.n == 2


def _key_state(w, tag):
    base = w._base if w._base is not None else w
    return (id(base), tag, w.storage_offset(), tuple(w.shape), tuple(w.stride())), (base.data_ptr(), base._version)


def test_dead_or_foreign_weak_reference_misses():
    """an entry under the live key with equal (address, version) state but a weak reference that is dead, or that names another
    object, is what a recycled id() leaves behind: it must not answer"""
    w, b = _w(4), Build()
    key, state = _key_state(w, TAG)
    gone = _w(5)
    dead = weakref.ref(gone)
    del gone
    gc.collect()
    assert dead() is None
    ops._weight_cache[key] = (dead, state, "stale-dead")
    assert ops._cached_weight_op(w, TAG, b) == ("b", 1)
    other = _w(6)
    ops._weight_cache[key] = (weakref.ref(other), state, "stale-foreign")
    assert ops._cached_weight_op(w, TAG, b) == ("b", 2)
    assert ops._cached_weight_op(w, TAG, b) == ("b", 2) and b.n == 2  # (the rebuilt entry is a proper one)
    # equal identity, another state: the two halves of `state` each
    ops._weight_cache[key] = (weakref.ref(w), (state[0] + 4, state[1]), "stale-address")
    assert ops._cached_weight_op(w, TAG, b) == ("b", 3)
    ops._weight_cache[key] = (weakref.ref(w), (state[0], state[1] + 1), "stale-version")
    assert ops._cached_weight_op(w, TAG, b) == ("b", 4)


def test_eviction_keeps_the_bound_and_drops_dead_entries_first():
    N = ops._WEIGHT_CACHE_MAX
    assert N == 512
    dead_n = 8
    doomed = [_w(100 + i, (1, 1, 1, 1)) for i in range(dead_n)]
    for i, t in enumerate(doomed):
        assert ops._cached_weight_op(t, TAG, Build(f"doomed{i}")) == (f"doomed{i}", 1)
    live = [_w(200 + i, (1, 1, 1, 1)) for i in range(N + 1)]
    builds = [Build(f"live{i}") for i in range(N + 1)]
    for i in range(N - dead_n):
        assert ops._cached_weight_op(live[i], TAG, builds[i]) == (f"live{i}", 1)
        assert len(ops._weight_cache) <= N
    assert len(ops._weight_cache) == N
    del doomed, t
    gc.collect()
    # the cache is full, eight of its entries are dead: the next insertion drops exactly those and every live entry survives
    i = N - dead_n
    assert ops._cached_weight_op(live[i], TAG, builds[i]) == (f"live{i}", 1)
    assert len(ops._weight_cache) == N - dead_n + 1
    for j in range(i + 1):
        assert ops._cached_weight_op(live[j], TAG, builds[j]) == (f"live{j}", 1), "a live entry was dropped while dead ones were there"
    # fill up with live bases only, then one more: the bound holds and every call still returns its own build's value
    for i in range(N - dead_n + 1, N + 1):
        assert ops._cached_weight_op(live[i], TAG, builds[i]) == (f"live{i}", 1)
        assert len(ops._weight_cache) <= N
    for i in range(N + 1):
        got = ops._cached_weight_op(live[i], TAG, builds[i])
        assert got == (f"live{i}", builds[i].n), f"base {i} got another base's value: {got}"
        assert len(ops._weight_cache) <= N
    assert ops._cached_weight_op(live[0], TAG, builds[0]) == ("live0", builds[0].n)


def test_cache_switched_off_builds_every_time_and_stores_nothing(monkeypatch):
    w, b = _w(7), Build()
    monkeypatch.setattr(ops, "WEIGHT_CACHE", False)
    assert [ops._cached_weight_op(w, TAG, b) for _ in range(3)] == [("b", 1), ("b", 2), ("b", 3)]
    assert len(ops._weight_cache) == 0
    # an entry from before the switch neither answers nor is replaced while it is off
    monkeypatch.setattr(ops, "WEIGHT_CACHE", True)
    kept = ops._cached_weight_op(w, TAG, b)
    monkeypatch.setattr(ops, "WEIGHT_CACHE", False)
    assert ops._cached_weight_op(w, TAG, b) == ("b", 5)
    monkeypatch.setattr(ops, "WEIGHT_CACHE", True)
    assert ops._cached_weight_op(w, TAG, b) is kept and b.n == 5


def test_data_write_announced_by_clear_rebuilds():
    """the documented contract: `.data.copy_` bumps no version and moves no address; after clear_weight_cache() the next call
    builds.  (Without the clear the result is unspecified and not asserted.)"""
    w, b = torch.nn.Parameter(_w(8)), Build()
    ops._cached_weight_op(w, TAG, b)
    w.data.copy_(_w(9))
    ops.clear_weight_cache()
    assert len(ops._weight_cache) == 0
    assert ops._cached_weight_op(w, TAG, b) == ("b", 2)


# ----------------------------------------------------------------------------------------------------------------- faces caches
QUAD = [[0, 1, 2], [0, 2, 3]]                      # four vertices, two faces sharing the edge 0-2
FAN = [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]]  # five vertices, four faces around vertex 0


def _tables(faces, V):
    """(int32 faces, CSR offsets, CSR entries, edge adjacency) as the two caches answer for `faces` now"""
    f32, off, ent = render._topology(faces, V, torch.device("cpu"))
    return [t.clone() for t in (f32, off, ent, antialias.edge_adjacency(faces))]


def _assert_fresh(faces, V, what):
    got, want = _tables(faces, V), _tables(faces.clone(), V)
    for name, g, w in zip(("faces", "csr offsets", "csr entries", "edge adjacency"), got, want):
        assert g.shape == w.shape and torch.equal(g, w), f"{what}: stale {name}: {g.tolist()} instead of {w.tolist()}"
    return got


def _differs(a, b):
    return any(x.shape != y.shape or not torch.equal(x, y) for x, y in zip(a, b))


def test_faces_caches_hit():
    f = torch.tensor(FAN)
    a = render._topology(f, 5, torch.device("cpu"))
    b = render._topology(f, 5, torch.device("cpu"))
    assert all(x is y for x, y in zip(a, b))
    assert antialias.edge_adjacency(f) is antialias.edge_adjacency(f)
    assert hasattr(f, "_gif_csr") and hasattr(f, "_gif_edge_adj")


def test_faces_caches_follow_an_in_place_row_edit():
    f = torch.tensor(FAN)
    before = _assert_fresh(f, 5, "fan")
    f[3] = torch.tensor([1, 4, 3])
    after = _assert_fresh(f, 5, "row edit")
    assert _differs(before, after)
    f.copy_(f[:, [0, 2, 1]].clone())  # winding flip
    assert _differs(after, _assert_fresh(f, 5, "winding flip"))


def test_topology_follows_another_vertex_count():
    f = torch.tensor(QUAD)
    a = _assert_fresh(f, 4, "V 4")
    b = _assert_fresh(f, 7, "V 7")
    assert a[1].shape == (5,) and b[1].shape == (8,)
    assert _assert_fresh(f, 4, "V 4 again")[1].shape == (5,)


def test_faces_caches_batched_against_plain():
    f = torch.tensor(FAN)
    fb = torch.stack([f, f])
    plain, batched = _assert_fresh(f, 5, "[F,3]"), _assert_fresh(fb, 5, "[B,F,3]")
    assert not _differs(plain, batched)
    fb[0, 3] = torch.tensor([1, 4, 3])  # the topology of sample 0 is the batch's
    assert _differs(plain, _assert_fresh(fb, 5, "[B,F,3] row edit"))


def test_faces_caches_after_deepcopy():
    """copy.deepcopy copies the attributes with the tensor: the copy's cache must be validated against the COPY"""
    f = torch.tensor(FAN)
    for _ in range(4):
        f[3] = torch.tensor([1, 4, 3])
    _assert_fresh(f, 5, "fan, edited")  # tables of version 4
    g = copy.deepcopy(f)  # a younger counter, with f's tables
    assert hasattr(g, "_gif_csr") and hasattr(g, "_gif_edge_adj"), "deepcopy no longer copies attributes: this row tests nothing"
    assert g._version < f._version - 1
    while g._version < f._version - 1:
        torch.autograd.graph.increment_version(g)
    g[3] = torch.tensor([0, 4, 1])  # the copy reaches version 4 with other contents: the counter alone cannot tell it from f
    assert g._version == f._version
    _assert_fresh(g, 5, "deepcopy, edited")
    _assert_fresh(f, 5, "the original after its copy was edited")


def test_faces_caches_follow_a_data_swap_of_equal_size():
    """faces.data = other keeps the version counter: the address in the key notices"""
    f = torch.tensor(QUAD)
    before = _assert_fresh(f, 4, "quad")
    other = torch.tensor([[0, 1, 3], [1, 2, 3]])  # the other diagonal
    f.data = other
    assert _differs(before, _assert_fresh(f, 4, "data swap, equal F"))


def test_faces_caches_follow_a_data_swap_of_another_face_count():
    """a stale CSR of another face count would index a face-gradient array of another length on the device: host-only row"""
    f = torch.tensor(QUAD)
    before = _assert_fresh(f, 5, "quad")
    f.data = torch.tensor(FAN)
    after = _assert_fresh(f, 5, "data swap, another F")
    assert after[0].shape == (4, 3) and after[2].shape == (12,) and after[3].shape == (4, 3)
    f.data = torch.tensor(QUAD)
    assert not _differs(before, _assert_fresh(f, 5, "data swap back"))


def test_faces_data_write_announced_by_deleting_the_attribute():
    """the documented contract, as for the weights: a write through .data into the same storage is the caller's to announce"""
    f = torch.tensor(FAN)
    _assert_fresh(f, 5, "fan")
    f.data[3] = torch.tensor([1, 4, 3])
    del f._gif_csr, f._gif_edge_adj
    _assert_fresh(f, 5, "announced .data write")


def test_csr_matches_its_definition():
    """the tables the rows above compare are the right ones: every (face, corner) is listed once under its vertex, corner passes 1, 2, 0
    and faces ascending inside a vertex; the adjacency names the one other face across each edge"""
    f = torch.tensor(FAN)
    f32, off, ent = render._topology(f, 6, torch.device("cpu"))
    assert f32.dtype == torch.int32 and torch.equal(f32.long(), f)
    off, ent = off.numpy(), ent.numpy()
    assert off[0] == 0 and off[-1] == 12 and off[6] == off[5]  # (vertex 5 is in no face)
    for v in range(6):
        want = [fi * 4 + c for c in (1, 2, 0) for fi in range(4) if FAN[fi][c] == v]
        assert ent[off[v]:off[v + 1]].tolist() == want, v
    adj = antialias.edge_adjacency(f).numpy()
    for fi in range(4):
        for k in range(3):
            a, b = FAN[fi][(k + 1) % 3], FAN[fi][(k + 2) % 3]
            others = [g for g in range(4) if g != fi and a in FAN[g] and b in FAN[g]]
            assert adj[fi, k] == (others[0] if len(others) == 1 else -1), (fi, k)
    assert np.array_equal(adj, np.array([[-1, 1, 3], [-1, 2, 0], [-1, 3, 1], [-1, 0, 2]]))
