"""Label groups summarised on the device: vc_group_summary, vc_group_summary_dev and their vc_sharded_* forms.

The expectation is groups_common.py's numpy model of the header's contract (pinned against plain loops, and its crafted inputs
against the cases they are there for, by test_groups_cpu.py).  Every output is integer arithmetic, so every comparison is exact
equality: groups field by field, centroid bytes, rep_labels, group_index.  Everything runs on one device; N <= 8192."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import groups_common as GC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STALE = 0xDEADBEEF
WINDOWS = [None, GC.SMALL_WINDOW]       # the default (one window) and windows of 2048 sorted positions


def _make(vc, monkeypatch, codes, window=None, id_base=0, shards=0, capacity=None):
    """the knob is read when the handle is created"""
    if window is None:
        monkeypatch.delenv("VC_GROUP_WINDOW", raising=False)
    else:
        monkeypatch.setenv("VC_GROUP_WINDOW", str(window))
    bits, capacity = codes.shape[1] * 8, capacity or max(len(codes), 1)
    if shards:
        e = vc.ShardedEngine(bits, capacity=capacity, n_shards=shards, devices=[0], id_base=id_base)
    else:
        e = vc.Engine(bits, capacity=capacity, id_base=id_base)
    if len(codes):
        e.add_codes(codes)
    return e


def _buffer(n_words):
    import torch
    buf = torch.from_numpy(np.full(max(n_words, 1), STALE, dtype=np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    return buf


def _read(buf):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint32)


def _dev(store, labels, cap=None, want=(True, True, True), stream=None):
    """the device form on stale-filled buffers: (rc, G, (groups, centroids | None, rep_labels | None, group_index | None), raw buffers)"""
    import torch
    n, row = len(labels), store.bits // 32
    cap = n if cap is None else cap
    d_labels = torch.from_numpy(np.array(labels, dtype=np.uint32).view(np.int32)).cuda() if n else None
    torch.cuda.synchronize()
    d_groups = _buffer(6 * cap)
    d_cents, d_rep, d_gi = (_buffer(row * cap) if want[0] else None), (_buffer(n) if want[1] else None), (_buffer(n) if want[2] else None)
    ptr = lambda b: b.data_ptr() if b is not None else None
    rc, G = store.group_summary_dev(ptr(d_labels), cap, d_groups.data_ptr(), ptr(d_cents), ptr(d_rep), ptr(d_gi), stream=stream)
    raw = (_read(d_groups), None if d_cents is None else _read(d_cents), None if d_rep is None else _read(d_rep),
           None if d_gi is None else _read(d_gi))
    out = None
    if rc == 0:
        out = (raw[0][:6 * G].view(GC.GROUP_DTYPE).copy(),
               None if raw[1] is None else raw[1][:row * G].view(np.uint8).reshape(G, store.bits // 8).copy(),
               None if raw[2] is None else raw[2][:n].copy(), None if raw[3] is None else raw[3][:n].copy())
    return rc, G, out, raw


def _check_both_forms(store, codes, labels, id_base=0, what=None, want=None):
    want = want or GC.model(codes, labels, id_base)
    GC.same(store.group_summary(labels), want, (what, "host form"))
    rc, G, got, _ = _dev(store, labels)
    assert rc == 0 and G == len(want[0]), what
    GC.same(got, want, (what, "device form"))
    return want


# ---- 1. every tier, every code width, one window and four ----------------------------------------------------------------------------
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("bits", GC.WIDTHS)
def test_tiers_and_windows(vc, monkeypatch, bits, window):
    """sizes 1, 2, 3, 64, 65, 1024, 1025 and 2049 in one partition of uniform codes; at windows of 2048 a pair, a wave-tier group and
    a chunk of the big group lie astride a boundary and the big group's chunks start in two windows"""
    codes, labels = GC.tier_case(bits)
    with _make(vc, monkeypatch, codes, window) as store:
        _check_both_forms(store, codes, labels, what=(bits, window), want=GC.tier_expect(bits))


@pytest.mark.parametrize("window", WINDOWS)
def test_all_singletons_and_one_group(vc, monkeypatch, window):
    n, bits = 4097, 128
    codes = GC.uniform_codes(n, bits, 77)
    with _make(vc, monkeypatch, codes, window) as store:
        own = np.arange(n, dtype=np.uint32)
        want = _check_both_forms(store, codes, own[::-1].copy(), what="singletons, labels reversed")
        assert len(want[0]) == n and np.array_equal(want[2], own) and np.array_equal(want[1][::-1], codes)
        for value in (0, 1234, n - 1):
            want = _check_both_forms(store, codes, np.full(n, value, dtype=np.uint32), what=("one group", value))
            assert len(want[0]) == 1 and want[0]["size"][0] == n and want[0]["label"][0] == value


@pytest.mark.parametrize("shards", [0, 2])
def test_one_and_two_records(vc, monkeypatch, shards):
    """N = 1 sorts by zero key bits (no pass: the input pair is the result), N = 2 by one"""
    for n in (1, 2):
        codes = GC.uniform_codes(n, 64, 40 + n)
        with _make(vc, monkeypatch, codes, shards=shards, capacity=4) as store:
            for labels in ([[0]] if n == 1 else [[0, 0], [1, 0], [1, 1], [0, 1]]):
                want = _check_both_forms(store, codes, np.array(labels, dtype=np.uint32), what=labels)
                assert len(want[0]) == len(set(labels))


def test_two_calls_on_two_streams_without_a_wait_between(vc, monkeypatch):
    """the handle's buffers serve both calls: the second is ordered behind the first by the handle, not by the caller"""
    import torch
    codes, labels = GC.tier_case(64)
    n, want, ones = len(labels), GC.tier_expect(64), GC.model(GC.tier_case(64)[0], np.zeros(len(labels), np.uint32))
    with _make(vc, monkeypatch, codes, GC.SMALL_WINDOW) as store:
        side = torch.cuda.Stream()
        d_a, d_b = (torch.from_numpy(np.array(x, dtype=np.uint32).view(np.int32)).cuda() for x in (labels, np.zeros(n, np.uint32)))
        out = [[_buffer(6 * n), _buffer(2 * n), _buffer(n), _buffer(n)] for _ in range(2)]
        torch.cuda.synchronize()
        for _ in range(3):
            ra = store.group_summary_dev(d_a.data_ptr(), n, *[b.data_ptr() for b in out[0]], stream=None)
            rb = store.group_summary_dev(d_b.data_ptr(), n, *[b.data_ptr() for b in out[1]], stream=side.cuda_stream)
            assert ra == (0, len(want[0])) and rb == (0, 1)
        for got, exp in ((out[0], want), (out[1], ones)):
            G = len(exp[0])
            GC.same((_read(got[0])[:6 * G].view(GC.GROUP_DTYPE), _read(got[1])[:2 * G].view(np.uint8).reshape(G, 8), _read(got[2]), _read(got[3])), exp)


@pytest.mark.parametrize("id_base", [1_000_000, None])
def test_id_base(vc, monkeypatch, id_base):
    """ids above zero, and ids that end at 2^32 (labels with the top bit set)"""
    n = len(GC.tier_case(64)[1])
    id_base = (1 << 32) - n if id_base is None else id_base
    codes, labels = GC.tier_case(64, id_base)
    with _make(vc, monkeypatch, codes, GC.SMALL_WINDOW, id_base=id_base) as store:
        want = _check_both_forms(store, codes, labels, id_base, what=id_base, want=GC.tier_expect(64, id_base))
        assert want[0]["rep"].min() >= id_base and np.array_equal(want[3], GC.tier_expect(64)[3])


def test_labels_that_are_not_roots(vc, monkeypatch):
    """the same partition under other label values changes the groups' order and labels and nothing else"""
    n, bits = 3000, 256
    rng = np.random.default_rng(9)
    codes = GC.uniform_codes(n, bits, 10)
    part = rng.integers(0, 300, size=n)
    with _make(vc, monkeypatch, codes) as store:
        _, first, inverse = np.unique(part, return_index=True, return_inverse=True)
        roots = first.astype(np.uint32)[inverse]                                        # the smallest member: a root
        a = _check_both_forms(store, codes, roots, what="roots")
        other = rng.permutation(n)[:len(first)].astype(np.uint32)[inverse]              # any id, member or not
        b = _check_both_forms(store, codes, other, what="not roots")
        assert np.count_nonzero(other[other] != other) > 0
        assert np.array_equal(a[2], b[2]) and not np.array_equal(a[3], b[3])
        assert sorted(a[0]["rep"].tolist()) == sorted(b[0]["rep"].tolist())


# ---- 2. the optional outputs, the capacity protocol, the errors ----------------------------------------------------------------------
@pytest.mark.parametrize("window", WINDOWS)
def test_null_outputs_and_capacity(vc, monkeypatch, window):
    bits = 128
    codes, labels = GC.tier_case(bits)
    want = GC.tier_expect(bits)
    G, n = len(want[0]), len(labels)
    with _make(vc, monkeypatch, codes, window) as store:
        for missing in range(3):
            sel = tuple(i != missing for i in range(3))
            rc, g, got, _ = _dev(store, labels, want=sel)
            assert rc == 0 and g == G and got[1 + missing] is None
            GC.same(got, want, ("NULL", missing))
        rc, g, got, _ = _dev(store, labels, want=(False, False, False))
        assert rc == 0 and g == G
        GC.same(got, want, "groups alone")
        rc, g, got, raw = _dev(store, labels, cap=G - 1)
        assert rc == vc.VC_ERR_CAPACITY and g == G
        assert np.all(raw[0] == STALE) and np.all(raw[1] == STALE)                      # groups and centroids untouched
        assert np.all(raw[2] == STALE) and np.all(raw[3] == STALE)                      # ... and, as the header says, the other two
        rc, g, got, raw = _dev(store, labels, cap=G)
        assert rc == 0 and g == G
        GC.same(got, want, "cap == G")
        L, p = vc.load_library(), lambda a: a.ctypes.data_as(C.c_void_p)
        count = C.c_uint64(99)
        import torch
        d_labels = torch.from_numpy(labels.view(np.int32).copy()).cuda()
        torch.cuda.synchronize()                                                        # d_groups may be NULL at groups_cap == 0
        assert L.vc_group_summary_dev(store._h, d_labels.data_ptr(), 0, None, None, None, None, C.byref(count), None) == vc.VC_ERR_CAPACITY
        assert count.value == G
        groups = np.full(6 * n, STALE, dtype=np.uint32)
        assert L.vc_group_summary(store._h, p(labels), G - 1, p(groups), None, None, None, C.byref(count)) == vc.VC_ERR_CAPACITY
        assert count.value == G and np.all(groups == STALE)
        assert L.vc_group_summary(store._h, p(labels), G, p(groups), None, None, None, None) == vc.VC_OK
        assert np.array_equal(groups[:6 * G].view(GC.GROUP_DTYPE), want[0]) and np.all(groups[6 * G:] == STALE)


@pytest.mark.parametrize("shards", [0, 3])
def test_bad_labels_and_null_arguments(vc, monkeypatch, shards):
    n, bits, id_base = 2500, 64, 500
    codes = GC.uniform_codes(n, bits, 3)
    labels = (np.random.default_rng(4).integers(0, 40, size=n) + id_base).astype(np.uint32)
    L, p = vc.load_library(), lambda a: a.ctypes.data_as(C.c_void_p)
    with _make(vc, monkeypatch, codes, GC.SMALL_WINDOW, id_base=id_base, shards=shards, capacity=3000) as store:
        fn = L.vc_sharded_group_summary if shards else L.vc_group_summary
        fn_dev = L.vc_sharded_group_summary_dev if shards else L.vc_group_summary_dev
        want = _check_both_forms(store, codes, labels, id_base)
        for where, value in ((1700, id_base + n), (0, id_base - 1), (n - 1, 0xFFFFFFFF), (5, 0)):
            bad = labels.copy()
            bad[where] = value
            with pytest.raises(vc.VcError) as err:
                _dev(store, bad)
            assert err.value.code == vc.VC_ERR_INVALID
            with pytest.raises(vc.VcError) as err:
                store.group_summary(bad)
            assert err.value.code == vc.VC_ERR_INVALID and "outside the resident id range" in str(err.value)
            _check_both_forms(store, codes, labels, id_base, what=("after a bad label", value), want=want)
        groups, count = np.zeros(6 * n, dtype=np.uint32), C.c_uint64(99)
        assert fn(None, p(labels), n, p(groups), None, None, None, C.byref(count)) == vc.VC_ERR_INVALID
        assert fn(store._h, None, n, p(groups), None, None, None, C.byref(count)) == vc.VC_ERR_INVALID
        assert fn(store._h, p(labels), n, None, None, None, None, C.byref(count)) == vc.VC_ERR_INVALID
        assert fn_dev(store._h, None, n, None, None, None, None, C.byref(count), None) == vc.VC_ERR_INVALID
        assert count.value == 99 and not groups.any()


@pytest.mark.parametrize("shards", [0, 3])
def test_an_empty_store(vc, monkeypatch, shards):
    with _make(vc, monkeypatch, np.zeros((0, 8), np.uint8), shards=shards, capacity=100) as store:
        got = store.group_summary(np.zeros(0, np.uint32))
        GC.same(got, GC.model(np.zeros((0, 8), np.uint8), np.zeros(0, np.uint32)))
        fn = vc.load_library().vc_sharded_group_summary_dev if shards else vc.load_library().vc_group_summary_dev
        count = C.c_uint64(99)
        assert fn(store._h, None, 0, None, None, None, None, C.byref(count), None) == vc.VC_OK and count.value == 0


# ---- 3. cluster, summarise, keep the representatives --------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 3])
@pytest.mark.parametrize("grouper", ["dbscan", "cluster", "leaders"])
def test_end_to_end(vc, monkeypatch, grouper, shards):
    n, bits = 1500, 64
    codes = GC.clustered_codes(n, bits, 21)
    with _make(vc, monkeypatch, codes, GC.SMALL_WINDOW, shards=shards, capacity=1600) as store:
        if grouper == "dbscan":
            labels = store.dbscan_radius(6, 4)[0]
        elif grouper == "cluster":
            labels = store.cluster_radius(4)[0]
        else:
            labels = store.leaders_radius(6)[0]
        want = GC.model(codes, labels)
        G = len(want[0])
        assert 20 < G < n and want[0]["size"].max() > 8
        got = store.group_summary(labels)
        GC.same(got, want, grouper)
        assert np.count_nonzero(got[0]["rep"] != got[0]["label"]) > 0                   # the representative is not the smallest id
        n_kept, new_ids = store.retain(got[2], vc.RETAIN_ROOTS)
        assert n_kept == G == len(store)
        reps = np.sort(got[0]["rep"])
        assert np.array_equal(np.flatnonzero(new_ids != 0xFFFFFFFF), reps)
        kept = np.stack([store.get_code(i) for i in range(G)])
        assert np.array_equal(kept, codes[reps])                                        # the representatives' codes in id order


# ---- 4. streams and call history ------------------------------------------------------------------------------------------------------
def test_device_form_on_another_stream_and_call_history(vc, monkeypatch):
    """the host form, the device form on the null stream and on a non-default stream give the same bits; so does the same call
    before and after a larger one (N groups) and a smaller one (one group) on the same handle: every word of the handle's scratch is written before it is read"""
    import torch
    bits = 256
    codes, labels = GC.tier_case(bits)
    want, n = GC.tier_expect(bits), len(labels)
    with _make(vc, monkeypatch, codes, GC.SMALL_WINDOW) as store:
        first = _dev(store, labels)[2]
        GC.same(first, want, "before")
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            rc, G, got, _ = _dev(store, labels, stream=side.cuda_stream)
        GC.same(got, want, "side stream")
        _check_both_forms(store, codes, np.arange(n, dtype=np.uint32), what="larger")
        GC.same(_dev(store, labels)[2], want, "after the larger call")
        _check_both_forms(store, codes, np.zeros(n, dtype=np.uint32), what="smaller")
        again = _dev(store, labels)[2]
        GC.same(again, first, "after the smaller call")
        GC.same(store.group_summary(labels), want, "host form at the end")


# ---- 5. sharded -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("bits", [64, 512])
def test_sharded_equals_the_single_engine(vc, monkeypatch, bits, window):
    """three shards on one device; the members of every larger group lie in all three"""
    codes, labels = GC.tier_case(bits)
    n = len(labels)
    with _make(vc, monkeypatch, codes, window, shards=3, capacity=n + 100) as sharded, _make(vc, monkeypatch, codes, window) as single:
        want = _check_both_forms(sharded, codes, labels, what=("sharded", bits, window), want=GC.tier_expect(bits))
        GC.same(sharded.group_summary(labels), single.group_summary(labels), "bit for bit")
        GC.same(_dev(sharded, labels)[2], _dev(single, labels)[2], "device forms, bit for bit")
        bounds = [(n + 100) * g // 3 for g in (1, 2)]
        for g in np.flatnonzero(want[0]["size"] >= 63):
            members = np.flatnonzero(want[3] == g)
            assert len(set(np.searchsorted(bounds, members, side="right").tolist())) == 3


def test_host_layer_group_summary(vc, tmp_path):
    """Backend::group_summary on both backends through the drop-in layer (tests/cpp/groups_host_test.cc), then retain of rep_labels"""
    from verticut_amd import build as vb
    src = os.path.join(ROOT, "tests", "cpp", "groups_host_test.cc")
    exe = tmp_path / "groups_host_test"
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-o", str(exe), str(src), "-I", vb.HOST, "-L", vb.LIBDIR, "-lverticut_gpu",
                           "-Wl,-rpath," + vb.LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib", "-L/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    n = 48
    i, j = np.arange(n)[:, None], np.arange(8)[None, :]
    codes = ((i * 37 + j * 11 + (i % 5) * j) & 255).astype(np.uint8)
    groups, cents, rep_labels, _ = GC.model(codes, (np.arange(n) * 7) % 9)
    text = " ".join("%d:%d:%d:%d:%d:%s" % (g["label"], g["size"], g["rep"], g["rep_dist"], g["max_dist"], bytes(c).hex()) for g, c in zip(groups, cents))
    line = "%%s %d %s | %s | %d" % (len(groups), text, " ".join(str(x) for x in rep_labels), len(groups))
    assert out.stdout.split("\n")[:2] == [line % "engine", line % "sharded"]
