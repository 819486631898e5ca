"""vc_sharded_retain* on the GPU: three id-range shards on one device, capacity not divisible by 3.  After a removal the survivors
again fill shard 0, then shard 1, ...: the handle R (add all, build_index, retain) equals, shard for shard, a fresh sharded handle F
fed the survivors in order, and one Engine E of the survivors -- ranges and sizes, new_ids, codes, buckets, searches -- also after
more records are added and the index is updated.

The mask "nothing removed from shard 0": the shards fill in id order, so shard 0 is full whenever another shard holds a record, and a
full shard that loses nothing has no room to receive; it is the shard that the call must leave ALONE (route none) while its
neighbours lose, give and receive."""
import os
import re
import subprocess

import numpy as np
import pytest

import index_update_common as U
import retain_common as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("VC_MIH_BCODES", "VC_MIH_BENT", "VC_MIH_LINES", "VC_MIH_STREAM", "VC_MIH_UPDATE", "VC_MIH_RETAIN")
DB = (300, 20000)
N = sum(DB)
CAPACITY = 21001                    # shards of 7000, 7000, 7001 ids; the store holds 7000 + 7000 + 6300 records
BOUNDS = (0, 7000, 14000, 21001)
SHARDED_MASKS = ("middle_shard_emptied", "last_shard_only", "trailing_shards_empty", "shard0_untouched", "sparse", "none", "all")


def _mask(name, keys, bits, m):
    keep = np.ones(N, dtype=bool)
    if name == "middle_shard_emptied":
        keep[7000:14000] = False
    elif name == "last_shard_only":
        keep[14000::2] = False
    elif name == "trailing_shards_empty":
        keep[5000:] = False
        keep[1:5000:7] = False
    elif name == "shard0_untouched":
        keep[7000:] = R.mask("every_other", keys, bits, m)[7000:] & R.mask("whole_buckets", keys, bits, m)[7000:]
    else:
        keep = R.mask(name, keys, bits, m)
    return keep


def _clean_env(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("VC_MIH_TRACE", "1")


def _host_stats(st):
    return [(s.radius, s.n_results, s.n_main_reads, s.n_sub_reads, s.n_local_reads, s.n_candidates) for s in st]


def _shard_lines(err):
    found = re.findall(r"\[vc_sharded\] retained: shard=(\d+) n=(\d+) kept=(\d+) given=(\d+) arrived=(\d+) route=(\w+)\n", err)
    return [(int(g), int(n), int(k), int(gv), int(a), r) for g, n, k, gv, a, r in found]


def _shards(h, tmp_path, tag):
    """per shard: (id range, size, its code file's bytes)"""
    out = []
    for g in range(3):
        e = h.shard(g)
        p = tmp_path / ("%s%d.codes" % (tag, g))
        e.save_code_file(p)
        out.append((h.shard_range(g), len(e), open(p, "rb").read()))
        os.unlink(p)
    return out


def _results(vc, h, q, sharded):
    out = {}
    for name, mode in (("linear", vc.MODE_LINEAR), ("exact", vc.MODE_MIH_EXACT)):
        rows, cnt, st = h.search_knn(q, 10, mode=mode, with_stats=True)
        out[name] = (rows.tolist(), cnt.tolist())
        out[name + "_stats"] = _host_stats(st) if sharded else None
    for name, mode in (("radius_linear", vc.MODE_LINEAR), ("radius_mih", vc.MODE_MIH_EXACT)):
        out[name] = [a.tolist() for a in h.search_radius(q[:6], 2, mode=mode, cap_per_query=1 << 14)]
    lab, pairs, clusters = h.cluster_radius(2, mode=vc.MODE_MIH_EXACT)
    out["cluster"] = (lab.tolist(), pairs, clusters)
    return out


def _buckets(h, m, key_lists, single):
    out = []
    for t in range(m):
        for key in key_lists[t]:
            got = h.get_bucket(t, key, with_codes=False) if single else h.get_bucket(t, key)
            out.append(None if got is None else (got[0].tolist(), got[-1]))
    return out


def _same(a, b, stats=True):
    return all(a[k] == b[k] for k in a if stats or not k.endswith("_stats"))


def _same_as_engine(vc, res_r, res_e, e, q, flags, where):
    """the sharded store against ONE engine of the same records.  Linear rows, radius results and clusters are functions of the
    database alone.  The exact MIH loop stops shard by shard, so without VC_FLAG_GLOBAL_STOP its rows may break ties at the last
    distance differently from the single engine's: there the distances are compared; under the flag rows and statistics are the
    single engine's."""
    for name in ("linear", "radius_linear", "radius_mih", "cluster"):
        assert res_r[name] == res_e[name], (where, name)
    if flags:
        rows, cnt, st = e.search_knn(q, 10, mode=vc.MODE_MIH_EXACT, with_stats=True)
        assert res_r["exact"] == (rows.tolist(), cnt.tolist()) and res_r["exact_stats"] == _host_stats(st), where
    else:
        dist = lambda rows: [[v >> 32 for v in row] for row in rows]
        assert dist(res_r["exact"][0]) == dist(res_e["exact"][0]) and res_r["exact"][1] == res_e["exact"][1], where


def _run(vc, monkeypatch, capfd, tmp_path, bits, m, mk, id_base=0, flags=0):
    _clean_env(monkeypatch)
    codes, keys = R.db_codes(bits, m, *DB), R.db_keys(bits, m, *DB)
    keep = _mask(mk, keys, bits, m)
    K = int(keep.sum())
    surv, surv_keys = np.ascontiguousarray(codes[keep]), keys[keep]
    where = (bits, m, mk, id_base, flags)
    rng = np.random.default_rng(17)
    q = codes[rng.integers(0, N, 12)].copy()
    q[::2, 0] ^= 3
    mk_sharded = lambda: vc.ShardedEngine(bits, capacity=CAPACITY, n_shards=3, n_tables=m, devices=[0], flags=flags, id_base=id_base)
    r, f = mk_sharded(), mk_sharded()
    try:
        assert [r.shard_range(g) for g in range(3)] == [(id_base + BOUNDS[g], BOUNDS[g + 1] - BOUNDS[g]) for g in range(3)]
        r.add_codes(codes)
        r.build_index()
        capfd.readouterr()
        n_kept, new_ids = r.retain(keep.astype(np.uint32))
        lines = _shard_lines(capfd.readouterr().err)
        assert n_kept == K == len(r) and np.array_equal(new_ids, R.new_ids_model(keep, id_base)), where
        # what every shard must report: its own survivors, what it gave to earlier shards, what arrived
        kept = [int(keep[BOUNDS[g]: min(BOUNDS[g + 1], N)].sum()) for g in range(3)]
        size = [max(0, min(K, BOUNDS[g + 1]) - BOUNDS[g]) if K > BOUNDS[g] else 0 for g in range(3)]
        assert [(ln[0], ln[1], ln[2]) for ln in lines] == [(g, size[g], kept[g]) for g in range(3)], (where, lines)
        for g, n_g, k_g, given, arrived, route in lines:
            had = min(BOUNDS[g + 1], N) - BOUNDS[g]
            assert k_g - given + arrived == n_g, (where, lines)
            assert route == ("empty" if n_g == 0 else "update" if arrived else "none" if (k_g == had and not given) else "filter"), (where, lines)
        if mk == "shard0_untouched":
            assert lines[0][3:] == (0, 0, "none") and lines[1][4] > 0 and lines[1][3] == 0 and lines[2][3] > 0, lines
        if K == 0:
            assert all(len(r.shard(g)) == 0 for g in range(3)) and r.get_code(id_base) is None
            r.add_codes(codes[:9000])                         # the empty store lives on
            r.build_index()
            f.add_codes(codes[:9000])
            f.build_index()
            assert _same(_results(vc, r, q, True), _results(vc, f, q, True)), where
            return
        f.add_codes(surv)
        f.build_index()
        with vc.Engine(bits, capacity=CAPACITY, n_tables=m, id_base=id_base) as e:
            e.add_codes(surv)
            e.build_index()
            assert _shards(r, tmp_path, "r") == _shards(f, tmp_path, "f"), where
            for gid in sorted({0, K - 1, K, 6999, 7000, 7001, 13999, 14000, K // 2} & set(range(0, N + 1))):
                exp = surv[gid] if gid < K else None
                for h in (r, f, e):
                    got = h.get_code(id_base + gid)
                    assert (got is None) == (exp is None) and (exp is None or np.array_equal(got, exp)), (where, gid)
            key_lists = [sorted(set(keys[:, t].tolist()))[:: (1 if t == 0 else 5)] for t in range(m)]     # removed keys included
            br = _buckets(r, m, key_lists, False)
            assert br == _buckets(f, m, key_lists, False) and br == _buckets(e, m, key_lists, True), where
            res_r, res_f, res_e = _results(vc, r, q, True), _results(vc, f, q, True), _results(vc, e, q, False)
            assert _same(res_r, res_f), where
            _same_as_engine(vc, res_r, res_e, e, q, flags, where)
            # life goes on: the freed room is filled again
            added = codes[~keep][: CAPACITY - K][:3000]
            for h in (r, f, e):
                h.add_codes(added)
                h.update_index()
            assert len(r) == len(f) == K + len(added)
            assert _shards(r, tmp_path, "r") == _shards(f, tmp_path, "f"), where
            res_r, res_f, res_e = _results(vc, r, q, True), _results(vc, f, q, True), _results(vc, e, q, False)
            assert _same(res_r, res_f), where
            _same_as_engine(vc, res_r, res_e, e, q, flags, where)
    finally:
        r.close()
        f.close()


@pytest.mark.parametrize("bits,m", [(64, 4), (128, 4)])
@pytest.mark.parametrize("mk", SHARDED_MASKS)
def test_sharded_retain(vc, monkeypatch, capfd, tmp_path, bits, m, mk):
    _run(vc, monkeypatch, capfd, tmp_path, bits, m, mk)


def test_sharded_retain_with_an_id_base(vc, monkeypatch, capfd, tmp_path):
    _run(vc, monkeypatch, capfd, tmp_path, 64, 4, "middle_shard_emptied", id_base=3000000)


def test_sharded_retain_under_the_global_stop(vc, monkeypatch, capfd, tmp_path):
    _run(vc, monkeypatch, capfd, tmp_path, 128, 4, "sparse", flags=0x10)


def test_sharded_roots_kind_and_device_form(vc, monkeypatch, capfd, tmp_path):
    """labels of cluster_radius_dev on the root device fed to retain_dev: the representatives survive, in both sharded and single form"""
    import torch
    _clean_env(monkeypatch)
    bits, m, n = 64, 4, 6000
    from oracle import vc_oracle as vo
    codes = vo.gen_codes(n, bits, 91, kind=1, n_centres=n // 6, max_flips=2)
    with vc.ShardedEngine(bits, capacity=6500, n_shards=3, n_tables=m, devices=[0]) as r, vc.Engine(bits, capacity=6500, n_tables=m) as e:
        for h in (r, e):
            h.add_codes(codes)
            h.build_index()
        d_labels = torch.empty(n, dtype=torch.int32, device="cuda")
        d_map = torch.empty(n, dtype=torch.int32, device="cuda")
        r.cluster_radius_dev(4, d_labels.data_ptr(), mode=vc.MODE_MIH_EXACT)
        K = r.retain_dev(d_labels.data_ptr(), kind=vc.RETAIN_ROOTS, d_new_ids=d_map.data_ptr())
        torch.cuda.synchronize()
        labels = d_labels.cpu().numpy().view(np.uint32)
        keep = labels == np.arange(n, dtype=np.uint32)
        assert 1 < K == keep.sum() == len(r) < n
        assert np.array_equal(d_map.cpu().numpy().view(np.uint32), R.new_ids_model(keep, 0))
        assert e.retain(labels, kind=vc.RETAIN_ROOTS)[0] == K
        q = codes[:8]
        for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
            a, b = r.search_knn(q, 10, mode=mode), e.search_knn(q, 10, mode=mode)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert r.cluster_radius(4, mode=vc.MODE_MIH_EXACT)[0].tolist() == e.cluster_radius(4, mode=vc.MODE_MIH_EXACT)[0].tolist()


def test_sharded_retain_on_two_devices(vc, monkeypatch, capfd, tmp_path):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (vc_sharded_* across devices has not run on hardware yet: one-GPU boxes)")
    _clean_env(monkeypatch)
    bits, m = 64, 4
    codes, keys = R.db_codes(bits, m, *DB), R.db_keys(bits, m, *DB)
    keep = _mask("middle_shard_emptied", keys, bits, m) & R.mask("sparse", keys, bits, m)
    with vc.ShardedEngine(bits, capacity=CAPACITY, n_shards=3, n_tables=m, devices=[0, 1]) as r, vc.Engine(bits, capacity=CAPACITY, n_tables=m) as e:
        r.add_codes(codes)
        r.build_index()
        n_kept, new_ids = r.retain(keep.astype(np.uint32))
        assert n_kept == keep.sum() and np.array_equal(new_ids, R.new_ids_model(keep, 0))
        e.add_codes(codes[keep])
        e.build_index()
        for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
            a, b = r.search_knn(codes[:8], 10, mode=mode), e.search_knn(codes[:8], 10, mode=mode)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_sharded_errors(vc, monkeypatch):
    import ctypes as C
    _clean_env(monkeypatch)
    L = vc.load_library()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    codes = R.db_codes(64, 4, 0, 500)
    with vc.ShardedEngine(64, capacity=700, n_shards=3, n_tables=4, devices=[0]) as h:
        kept = C.c_uint64(99)
        assert L.vc_sharded_retain(h._h, None, 0, None, C.byref(kept)) == vc.VC_OK and kept.value == 0        # N == 0
        h.add_codes(codes)
        h.build_index()
        n = len(codes)
        sel = np.ones(n, dtype=np.uint32)
        sentinel = np.full(2 * n, 0xABCDEF01, dtype=np.uint32)
        kept = C.c_uint64(99)
        for i, call in enumerate((
            lambda: L.vc_sharded_retain(None, p(sel), 0, p(sentinel), C.byref(kept)),
            lambda: L.vc_sharded_retain(h._h, None, 0, p(sentinel), C.byref(kept)),
            lambda: L.vc_sharded_retain(h._h, p(sel), 2, p(sentinel), C.byref(kept)),
            lambda: L.vc_sharded_retain(h._h, p(sentinel), 0, p(sentinel[n - 1:]), C.byref(kept)),
            lambda: L.vc_sharded_retain_dev(h._h, None, 0, None, C.byref(kept), None),
            lambda: L.vc_sharded_retain_dev(h._h, p(sel), 7, None, C.byref(kept), None),
        )):
            assert call() == vc.VC_ERR_INVALID, i
            assert len(h) == n and kept.value == 99 and np.all(sentinel == 0xABCDEF01), i
        assert np.all(h.search_knn(codes[:4], 5, mode=vc.MODE_MIH_EXACT)[1] == 5)


def test_host_layer_retain(vc, tmp_path):
    """Backend::retain on both backends through the drop-in layer (tests/cpp/retain_test.cc): n_kept, the map, the bucket's new ids"""
    from verticut_amd import build as vb
    src = os.path.join(ROOT, "tests", "cpp", "retain_test.cc")
    exe = tmp_path / "retain_test"
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-o", str(exe), str(src), "-I", vb.HOST, "-L", vb.LIBDIR, "-lverticut_gpu",
                           "-Wl,-rpath," + vb.LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib", "-L/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    keep = [i % 3 != 0 for i in range(40)]
    new_id = {i: sum(keep[:i]) for i in range(40) if keep[i]}
    bucket = " ".join(str(new_id[i]) for i in range(0, 40, 4) if keep[i])
    assert out.stdout.split("\n")[:2] == ["engine kept %d bucket %s" % (sum(keep), bucket), "sharded kept %d bucket %s" % (sum(keep), bucket)]
