"""vc_retain* on the GPU: a store cut down to its survivors in place (handle R: add all, build_index, retain) is BIT FOR BIT the store
of the survivors (handle F: add survivors, build_index) -- codes, index (as saved files where a file is small enough, else bucket by
bucket and bitmap word by bitmap word), every search -- for every bucket situation of retain_common, every index layout, any call
history, both routes and both call forms.  The VC_MIH_TRACE line "index retained: ..." is the witness of the route a call took."""
import filecmp
import os
import re

import numpy as np
import pytest

import flag_routes_common as F
import index_update_common as U
import retain_common as R

pytestmark = pytest.mark.gpu

KNOBS = ("VC_MIH_BCODES", "VC_MIH_BENT", "VC_MIH_LINES", "VC_MIH_STREAM", "VC_MIH_UPDATE", "VC_MIH_RETAIN")
GONE = R.GONE


def _retain_lines(err):
    """the 'index retained' lines of a captured stderr -> [(n, removed, route, bent, bcodes, lines)]"""
    found = re.findall(r"\[vc_mih\] index retained: n=(\d+) removed=(\d+) route=(\w+) bent=(\w+) bcodes=([01]) lines=([01])\n", err)
    return [(int(n), int(a), r, b, int(bc), int(ln)) for n, a, r, b, bc, ln in found]


def _clean_env(monkeypatch, **env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("VC_MIH_TRACE", "1")
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _host_stats(st):
    return [(s.radius, s.n_results, s.n_main_reads, s.n_sub_reads, s.n_local_reads, s.n_candidates) for s in st]


def _same_files(a, b):
    same = filecmp.cmp(a, b, shallow=False)
    os.unlink(a)
    os.unlink(b)
    return same


def _same_codes(r, f, tmp_path):
    r.save_code_file(tmp_path / "r.codes")
    f.save_code_file(tmp_path / "f.codes")
    return _same_files(tmp_path / "r.codes", tmp_path / "f.codes")


def _watched_keys(bits, m, keys):
    """per table: the planted and the vanish-set keys that occur in the database (survivors or not)"""
    out = []
    for t in range(m):
        p = U.plan(bits, m, t)
        want = set((0,) + p.below + p.above + p.between + p.edges + ((p.empty_block,) if p.empty_block is not None else ())) | set(R.vanish_set(bits, m, t))
        out.append(sorted(want & set(keys[:, t].tolist())))
    return out


def _compare_views(r, f, bits, m, surv_keys, watched, id_base, where):
    """R against F and against the stable sort of the survivors: every surviving key's bucket in every table, the bitmap words around
    the watched keys (planted and vanished), absent keys with bitmap_test == 0 and no bucket"""
    s = bits // m
    words = (1 << s) // 32
    for t in range(m):
        col = surv_keys[:, t]
        order = np.argsort(col, kind="stable")
        present = set(col.tolist())
        for key in sorted(present):
            exp = (order[np.searchsorted(col[order], key, "left"): np.searchsorted(col[order], key, "right")] + id_base).astype(np.uint32)
            gr, gf = r.get_bucket(t, key, with_codes=False), f.get_bucket(t, key, with_codes=False)
            assert gr is not None and gf is not None, (where, t, key)
            assert gr[2] == gf[2] == len(exp) and np.array_equal(gr[0], exp) and np.array_equal(gf[0], exp), (where, t, key)
        for key in watched[t]:
            w0 = max(0, (key >> 5) - 1)
            cnt = min(3, words - w0)
            assert np.array_equal(r.bitmap_read(t, w0, cnt), f.bitmap_read(t, w0, cnt)), (where, t, key)
            assert r.bitmap_test(t, key) == f.bitmap_test(t, key) == int(key in present), (where, t, key)
            if key not in present:
                assert r.get_bucket(t, key) is None and f.get_bucket(t, key) is None, (where, t, key)
        for key in (2, 5, (1 << s) - 2, (1 << (s - 1)) + 1):
            if key not in present:
                assert r.bitmap_test(t, key) == 0 and f.bitmap_test(t, key) == 0 and r.get_bucket(t, key) is None, (where, t, key)


def _compare_index(r, f, tmp_path, bits, m, surv_keys, watched, id_base, where):
    if (bits, m) in U.FILE_SHAPES:
        r.save_index(tmp_path / "r.vcidx")
        f.save_index(tmp_path / "f.vcidx")
        assert _same_files(tmp_path / "r.vcidx", tmp_path / "f.vcidx"), where
    else:
        _compare_views(r, f, bits, m, surv_keys, watched, id_base, where)


def _no_index(vc, e, q):
    with pytest.raises(vc.VcError) as ei:
        e.search_knn(q, 1, mode=vc.MODE_MIH_EXACT)
    return ei.value.code == vc.VC_ERR_STATE


def _retain_and_compare(vc, capfd, tmp_path, bits, m, codes, keys, keep, where, id_base=0, sel=None, kind=None, route="filter"):
    """R: add all, build, retain; F: add survivors, build; n_kept, size, new_ids, codes, index, trace"""
    n, K = len(codes), int(keep.sum())
    if sel is None:
        sel, kind = keep.astype(np.uint32), vc.RETAIN_MASK
    with vc.Engine(bits, capacity=n, n_tables=m, id_base=id_base) as r, vc.Engine(bits, capacity=n, n_tables=m, id_base=id_base) as f:
        r.add_codes(codes)
        r.build_index()
        capfd.readouterr()
        n_kept, new_ids = r.retain(sel, kind=kind)
        lines = _retain_lines(capfd.readouterr().err)
        assert n_kept == K and len(r) == K, (where, n_kept, K)
        assert np.array_equal(new_ids, R.new_ids_model(keep, id_base)), where
        if K == 0:
            assert lines == [] and _no_index(vc, r, codes[:1]), (where, lines)
            assert r.get_code(id_base) is None
            return
        assert len(lines) == 1 and lines[0][:3] == (K, n - K, "none" if K == n else route), (where, lines)
        f.add_codes(codes[keep])
        f.build_index()
        assert _same_codes(r, f, tmp_path), where
        assert np.array_equal(r.get_code(id_base + K - 1), codes[keep][-1]) and r.get_code(id_base + K) is None, where
        _compare_index(r, f, tmp_path, bits, m, keys[keep], _watched_keys(bits, m, keys), id_base, where)


DB_CASES = [c for c in R.cases() if c[2] == "db"]
SWEEP_CASES = [c for c in R.cases() if c[2] == "sweep"]


def _case_id(c):
    return "%d-%d-%s-%s-%s" % (c[0], c[1], c[2], "+".join(map(str, c[3])) if c[2] == "db" else c[3], c[4])


@pytest.mark.parametrize("bits,m,kind,size,mk", DB_CASES + SWEEP_CASES, ids=[_case_id(c) for c in DB_CASES + SWEEP_CASES])
def test_retained_index_is_the_built_index(vc, monkeypatch, capfd, tmp_path, bits, m, kind, size, mk):
    """1. + 2. every (shape, database, mask) and the size sweep: n_kept, size, new_ids, code file, index, trace"""
    _clean_env(monkeypatch)
    codes, keys = R.case_codes(bits, m, kind, size), R.case_keys(bits, m, kind, size)
    _retain_and_compare(vc, capfd, tmp_path, bits, m, codes, keys, R.mask(mk, keys, bits, m), (bits, m, kind, size, mk))


@pytest.mark.parametrize("bits,m", [(64, 4), (128, 4)])
@pytest.mark.parametrize("mk", ["whole_buckets", "every_other"])
def test_retain_with_an_id_base(vc, monkeypatch, capfd, tmp_path, bits, m, mk):
    """3. id_base != 0: the tables hold local ids, new_ids and the views are global"""
    _clean_env(monkeypatch)
    codes, keys = R.db_codes(bits, m, 300, 20000), R.db_keys(bits, m, 300, 20000)
    _retain_and_compare(vc, capfd, tmp_path, bits, m, codes, keys, R.mask(mk, keys, bits, m), (bits, m, mk, "id_base"), id_base=1000000)


@pytest.mark.parametrize("bits,m,id_base", [(64, 4, 0), (64, 2, 0), (128, 4, 777000)])
def test_roots_kind_on_crafted_labels(vc, monkeypatch, capfd, tmp_path, bits, m, id_base):
    """4. VC_RETAIN_ROOTS: a survivor carries its own id, a removed record any smaller id -- the result of the equivalent mask"""
    _clean_env(monkeypatch)
    codes, keys = R.db_codes(bits, m, 300, 20000), R.db_keys(bits, m, 300, 20000)
    keep = R.mask("sparse", keys, bits, m) & R.mask("every_other", keys, bits, m)
    keep[0] = True                                            # (record 0 has no smaller id to point at)
    rng = np.random.default_rng(5)
    own = id_base + np.arange(len(codes), dtype=np.int64)
    labels = np.where(keep, own, id_base + (rng.random(len(codes)) * np.arange(len(codes))).astype(np.int64)).astype(np.uint32)
    assert np.array_equal(labels == own, keep)
    _retain_and_compare(vc, capfd, tmp_path, bits, m, codes, keys, keep, (bits, m, "roots"), id_base=id_base, sel=labels, kind=vc.RETAIN_ROOTS)


def _near_duplicate_db(oracle, bits, n):
    return oracle.gen_codes(n, bits, 91, kind=1, n_centres=n // 6, max_flips=2)


@pytest.mark.parametrize("bits,m", [(64, 4), (128, 4)])
def test_cluster_labels_to_retain_without_leaving_the_device(vc, oracle, monkeypatch, capfd, tmp_path, bits, m):
    """4. cluster_radius_dev labels fed straight to retain_dev: F built from codes[labels == ids]; the map carries the labels over"""
    import torch
    _clean_env(monkeypatch)
    n = 6000
    codes = _near_duplicate_db(oracle, bits, n)
    with vc.Engine(bits, capacity=n, n_tables=m) as r, vc.Engine(bits, capacity=n, n_tables=m) as f:
        r.add_codes(codes)
        r.build_index()
        d_labels = torch.empty(n, dtype=torch.int32, device="cuda")
        d_map = torch.empty(n, dtype=torch.int32, device="cuda")
        r.cluster_radius_dev(4, d_labels.data_ptr(), mode=vc.MODE_MIH_EXACT)
        capfd.readouterr()
        K = r.retain_dev(d_labels.data_ptr(), kind=vc.RETAIN_ROOTS, d_new_ids=d_map.data_ptr())
        torch.cuda.synchronize()
        labels = d_labels.cpu().numpy().view(np.uint32)
        keep = labels == np.arange(n, dtype=np.uint32)
        assert 1 < keep.sum() < n and K == keep.sum() == len(r)
        assert [ln[:3] for ln in _retain_lines(capfd.readouterr().err)] == [(K, n - K, "filter")]
        new_ids = d_map.cpu().numpy().view(np.uint32)
        assert np.array_equal(new_ids, R.new_ids_model(keep, 0))
        assert np.all(new_ids[labels] != GONE)                # every record's representative survived: labels carry over
        f.add_codes(codes[keep])
        f.build_index()
        assert _same_codes(r, f, tmp_path)
        r.save_index(tmp_path / "r.vcidx")
        f.save_index(tmp_path / "f.vcidx")
        assert _same_files(tmp_path / "r.vcidx", tmp_path / "f.vcidx")
        lr, lf = r.cluster_radius(4, mode=vc.MODE_MIH_EXACT), f.cluster_radius(4, mode=vc.MODE_MIH_EXACT)
        assert np.array_equal(lr[0], lf[0]) and lr[1:] == lf[1:]


# ---------------------------------------------------------------- 5. searches
def _queries(codes, keep, rng):
    """16 queries: survivors, removed records, and both with a few flipped bits"""
    rows = np.concatenate([rng.choice(np.nonzero(keep)[0], 8), rng.choice(np.nonzero(~keep)[0], 8)])
    q = codes[rows].copy()
    for i in range(len(q)):
        for b in rng.choice(codes.shape[1] * 8, size=i % 4, replace=False):
            q[i, b // 8] ^= np.uint8(1 << (b % 8))
    return q


def _all_searches(vc, h, q, n, radius):
    """every search call of the store with what it returns, as comparable lists"""
    out = {}
    for name, mode, k in (("linear", vc.MODE_LINEAR, 10), ("exact", vc.MODE_MIH_EXACT, 10), ("approx", vc.MODE_MIH_APPROX, 5), ("exact_big", vc.MODE_MIH_EXACT, 300)):
        rows, cnt, st = h.search_knn(q, k, mode=mode, with_stats=True)
        out[name] = (rows.tolist(), cnt.tolist(), _host_stats(st))
    for name, mode in (("radius_linear", vc.MODE_LINEAR), ("radius_mih", vc.MODE_MIH_EXACT)):
        out[name] = [a.tolist() for a in h.search_radius(q, radius, mode=mode, cap_per_query=1 << 15)]
    ids = np.array([h.id_base, h.id_base + n // 2, h.id_base + n - 1, h.id_base + n, 3], dtype=np.uint32)
    rows, cnt, st = h.search_knn_ids(ids, 7, mode=vc.MODE_MIH_EXACT, id_flags=vc.IDS_EXCLUDE_SELF, with_stats=True)
    out["knn_ids"] = (rows.tolist(), cnt.tolist(), _host_stats(st))
    out["radius_ids"] = [a.tolist() for a in h.search_radius_ids(ids, radius, mode=vc.MODE_MIH_EXACT, id_flags=vc.IDS_ONLY_GREATER, cap_per_query=1 << 15)]
    lab, pairs, clusters = h.cluster_radius(radius, mode=vc.MODE_MIH_EXACT)
    out["cluster"] = (lab.tolist(), pairs, clusters)
    return out


def _brute_knn(oracle, codes, q, k, id_base=0):
    out = []
    for i in range(len(q)):
        d = oracle.np_distances(codes, q[i])
        packed = np.sort(oracle.pack(d, np.arange(len(codes), dtype=np.uint64) + id_base))
        out.append(packed[:k].tolist())
    return out


@pytest.mark.parametrize("bits,m", [(64, 2), (64, 4), (128, 4), (256, 8)])
@pytest.mark.parametrize("mk", ["every_other", "whole_buckets", "sparse"])
def test_searches_after_the_call(vc, oracle, monkeypatch, bits, m, mk):
    """5. R against F bit for bit -- k-NN linear / exact / approximate with statistics, radius, by-id k-NN and radius, clustering --
    and the linear rows against a numpy brute force over the survivors"""
    _clean_env(monkeypatch)
    codes, keys = R.db_codes(bits, m, 300, 20000), R.db_keys(bits, m, 300, 20000)
    keep = R.mask(mk, keys, bits, m)
    K = int(keep.sum())
    q = _queries(codes, keep, np.random.default_rng(bits + m))
    with vc.Engine(bits, capacity=len(codes), n_tables=m) as r, vc.Engine(bits, capacity=len(codes), n_tables=m) as f:
        r.add_codes(codes)
        r.build_index()
        assert r.retain(keep.astype(np.uint32))[0] == K
        f.add_codes(codes[keep])
        f.build_index()
        got, exp = _all_searches(vc, r, q, K, 2), _all_searches(vc, f, q, K, 2)
        for name in exp:
            assert got[name] == exp[name], (bits, m, mk, name)
        brute = _brute_knn(oracle, codes[keep], q, 10)
        for i in range(len(q)):
            assert got["linear"][0][i] == brute[i] and got["linear"][1][i] == 10, (bits, m, mk, i)


# ---------------------------------------------------------------- 6. every layout
def _layout_cells():
    import test_index_policy_gpu as P
    return [c for c in P.CELLS if (c[0], c[1]) in ((64, 2), (128, 4), (64, 4), (128, 8))]


def _knn_expect(vo, codes, q, m, k):
    """[nq] (canonical row, statistics) of MihOracle.find over `codes`"""
    mo = vo.MihOracle(codes, m, key_mode=1)
    out = []
    for i in range(len(q)):
        ores, ost = mo.find(q[i], k, stop_mult=min(m, 4))
        row, reachable = F.canonical_mih(vo, codes, q[i], m, k, ost.radius, False)
        assert reachable == ost.n_distinct and ost.n_main_reads == 0
        F.check_contract(row, ores)
        out.append((row, (ost.radius, ost.n_results, 0, ost.n_sub_reads, ost.n_local_reads, ost.n_distinct)))
    mo.close()
    return out


@pytest.mark.parametrize("bits,m,layout", _layout_cells(), ids=["%d-%d-%s" % (b, m, "-".join(ly)) for b, m, ly in _layout_cells()])
def test_every_layout_after_a_retain(vc, oracle, monkeypatch, capfd, bits, m, layout):
    """6. the knob routes of test_index_policy_gpu, on its database with every third record removed: the trace shows the layout the
    knobs name (records filtered, not gathered again); exact k-NN (k = 20), approximate k-NN and a radius search give handle F's
    rows, counts and statistics, and the exact rows and statistics are MihOracle's over the survivors"""
    import test_index_policy_gpu as P
    _clean_env(monkeypatch, **dict(P.LAYOUT_ENV[ly] for ly in layout))
    codes, base, q = P._data(oracle, bits, m)
    where = (bits, m, layout)
    bcodes, bent, lines = P._cell_layout(bits, m, layout)
    keep = np.arange(P.N) % 3 != 1
    K = int(keep.sum())
    surv = np.ascontiguousarray(codes[keep])
    with vc.Engine(bits, capacity=P.N, n_tables=m) as r, vc.Engine(bits, capacity=P.N, n_tables=m) as f:
        r.add_codes(codes)
        r.build_index()
        capfd.readouterr()
        assert r.retain(keep.astype(np.uint32), with_map=False) == (K, None)
        assert _retain_lines(capfd.readouterr().err) == [(K, P.N - K, "filter", "filter" if bent else "0", bcodes, lines)], where
        f.add_codes(surv)
        f.build_index()
        assert P._layout_line(capfd.readouterr().err, "built")[4:] == (bcodes, bent, lines), where
        nq = 8
        got = r.search_knn(q[:nq], P.K_SMALL, mode=vc.MODE_MIH_EXACT, with_stats=True)
        exp = f.search_knn(q[:nq], P.K_SMALL, mode=vc.MODE_MIH_EXACT, with_stats=True)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and _host_stats(got[2]) == _host_stats(exp[2]), where
        for i, (row, st) in enumerate(_knn_expect(oracle, surv, q[:nq], m, P.K_SMALL)):
            assert got[1][i] == len(row) and np.array_equal(got[0][i, : len(row)], row) and _host_stats(got[2])[i] == st, (where, i)
        got = r.search_knn(q, 5, mode=vc.MODE_MIH_APPROX, with_stats=True)
        exp = f.search_knn(q, 5, mode=vc.MODE_MIH_APPROX, with_stats=True)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and _host_stats(got[2]) == _host_stats(exp[2]), where
        d = oracle.np_distances(surv, base)
        for rad in (0, m, 2 * m + 2):
            a = r.search_radius(base[None, :], rad, mode=vc.MODE_MIH_EXACT, cap_per_query=1 << 15)[0]
            b = f.search_radius(base[None, :], rad, mode=vc.MODE_MIH_EXACT, cap_per_query=1 << 15)[0]
            ids = np.nonzero(d <= rad)[0]
            assert np.array_equal(a, b) and np.array_equal(a, np.sort(oracle.pack(d[ids], ids.astype(np.uint64)))), (where, rad)


# ---------------------------------------------------------------- 7. the rebuild route
@pytest.mark.parametrize("bits,m", [(64, 4), (64, 2)])
def test_rebuild_route_gives_the_same_file(vc, monkeypatch, capfd, tmp_path, bits, m):
    """7. VC_MIH_RETAIN=0: the call compacts the columns and rebuilds (the trace says so); the file is the filter route's"""
    codes, keys = R.sweep_codes(bits, m, 4097), R.sweep_keys(bits, m, 4097)
    keep = R.mask("whole_buckets", keys, bits, m) & R.mask("sparse", keys, bits, m)
    K = int(keep.sum())
    paths = {}
    for route, env in (("filter", {}), ("rebuild", {"VC_MIH_RETAIN": "0"})):
        _clean_env(monkeypatch, **env)
        with vc.Engine(bits, capacity=len(codes), n_tables=m) as e:
            e.add_codes(codes)
            e.build_index()
            capfd.readouterr()
            assert e.retain(keep.astype(np.uint32))[0] == K
            assert [ln[:3] for ln in _retain_lines(capfd.readouterr().err)] == [(K, len(codes) - K, route)]
            paths[route] = tmp_path / (route + ".vcidx")
            e.save_index(paths[route])
    assert _same_files(paths["filter"], paths["rebuild"])


# ---------------------------------------------------------------- 8. life goes on
@pytest.mark.parametrize("bits,m", [(64, 4), (64, 2)])
def test_life_goes_on(vc, monkeypatch, capfd, tmp_path, bits, m):
    """8. retain, add_codes, update_index == a build of survivors + added; two retains == one with the composed mask; the saved
    index of a retained handle loads into a fresh handle holding the survivors (the digest matches)"""
    _clean_env(monkeypatch)
    codes, keys = R.db_codes(bits, m, 300, 20000), R.db_keys(bits, m, 300, 20000)
    k1 = R.mask("sparse", keys, bits, m) & R.mask("whole_buckets", keys, bits, m)
    k2 = R.mask("every_other", keys[k1], bits, m)
    both = k1.copy()
    both[np.nonzero(k1)[0][~k2]] = False
    added = codes[~k1][:700]                                  # removed records come back, at the end
    with vc.Engine(bits, capacity=len(codes), n_tables=m) as r, vc.Engine(bits, capacity=len(codes), n_tables=m) as f:
        r.add_codes(codes)
        r.build_index()
        assert r.retain(k1.astype(np.uint32))[0] == k1.sum()
        assert r.retain(k2.astype(np.uint32))[0] == both.sum() == len(r)
        f.add_codes(codes[both])
        f.build_index()
        r.save_index(tmp_path / "r.vcidx")
        f.save_index(tmp_path / "f.vcidx")
        assert filecmp.cmp(tmp_path / "r.vcidx", tmp_path / "f.vcidx", shallow=False)
        os.unlink(tmp_path / "f.vcidx")
        with vc.Engine(bits, capacity=len(codes), n_tables=m) as third:
            third.add_codes(codes[both])
            third.load_index(tmp_path / "r.vcidx")            # (accepted: the digest of the survivors' codes matches)
            a, b = third.search_knn(codes[:4], 10, mode=vc.MODE_MIH_EXACT), f.search_knn(codes[:4], 10, mode=vc.MODE_MIH_EXACT)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        os.unlink(tmp_path / "r.vcidx")
        r.add_codes(added)
        assert _no_index(vc, r, codes[:1])
        capfd.readouterr()
        r.update_index()
        assert "route=merge" in capfd.readouterr().err
    with vc.Engine(bits, capacity=len(codes), n_tables=m) as r2, vc.Engine(bits, capacity=len(codes), n_tables=m) as f2:
        r2.add_codes(codes)
        r2.build_index()
        r2.retain(both.astype(np.uint32))
        r2.add_codes(added)
        r2.update_index()
        f2.add_codes(np.concatenate([codes[both], added]))
        f2.build_index()
        assert _same_codes(r2, f2, tmp_path)
        r2.save_index(tmp_path / "r.vcidx")
        f2.save_index(tmp_path / "f.vcidx")
        assert _same_files(tmp_path / "r.vcidx", tmp_path / "f.vcidx")


# ---------------------------------------------------------------- 9. history independence
@pytest.mark.parametrize("bits,m", [(64, 4), (128, 4)])
def test_history_independence(vc, monkeypatch, bits, m):
    """9. a handle that answered large k-NN, radius and cluster calls before the retain returns, after it, the bits F returns for the
    same calls; repeating the calls returns the same bits"""
    _clean_env(monkeypatch)
    codes, keys = R.db_codes(bits, m, 300, 20000), R.db_keys(bits, m, 300, 20000)
    keep = R.mask("second_half", keys, bits, m) & R.mask("sparse", keys, bits, m)
    K = int(keep.sum())
    q = _queries(codes, keep, np.random.default_rng(9))
    with vc.Engine(bits, capacity=len(codes), n_tables=m) as r, vc.Engine(bits, capacity=len(codes), n_tables=m) as f:
        r.add_codes(codes)
        r.build_index()
        r.search_knn(np.tile(q, (40, 1)), 2000, mode=vc.MODE_MIH_EXACT)
        r.search_knn(np.tile(q, (8, 1)), 500, mode=vc.MODE_LINEAR)
        r.search_radius(q, 6, mode=vc.MODE_MIH_EXACT, cap_per_query=1 << 15)
        r.cluster_radius(3, mode=vc.MODE_MIH_EXACT)
        _all_searches(vc, r, q, len(codes), 3)
        assert r.retain(keep.astype(np.uint32))[0] == K
        f.add_codes(codes[keep])
        f.build_index()
        exp = _all_searches(vc, f, q, K, 2)
        first, again = _all_searches(vc, r, q, K, 2), _all_searches(vc, r, q, K, 2)
        for name in exp:
            assert first[name] == exp[name] and again[name] == exp[name], (bits, m, name)


# ---------------------------------------------------------------- 10. states and errors
def test_states(vc, monkeypatch, capfd, tmp_path):
    """10. a stale index is dropped; no index before means none after; mask `none` leaves an empty handle that lives on; N == 0"""
    _clean_env(monkeypatch)
    bits, m = 64, 4
    codes, keys = R.db_codes(bits, m, 300, 20000), R.db_keys(bits, m, 300, 20000)
    keep = R.mask("every_other", keys, bits, m)
    half = len(codes) // 2
    with vc.Engine(bits, capacity=len(codes), n_tables=m) as e, vc.Engine(bits, capacity=len(codes), n_tables=m) as f:
        f.add_codes(codes[keep])
        f.build_index()
        f.save_index(tmp_path / "f.vcidx")
        # stale
        e.add_codes(codes[:half])
        e.build_index()
        e.add_codes(codes[half:])
        capfd.readouterr()
        assert e.retain(keep.astype(np.uint32))[0] == keep.sum()
        assert _retain_lines(capfd.readouterr().err) == [] and _no_index(vc, e, codes[:1])
        assert _same_codes(e, f, tmp_path)
        e.build_index()
        e.save_index(tmp_path / "e.vcidx")
        assert filecmp.cmp(tmp_path / "e.vcidx", tmp_path / "f.vcidx", shallow=False)
        # nothing removed: nothing changes, the index stays
        capfd.readouterr()
        n_kept, ids = e.retain(np.ones(len(e), dtype=np.uint32))
        assert n_kept == len(e) and np.array_equal(ids, np.arange(len(e), dtype=np.uint32))
        assert [ln[:3] for ln in _retain_lines(capfd.readouterr().err)] == [(len(e), 0, "none")]
        e.save_index(tmp_path / "e.vcidx")
        assert _same_files(tmp_path / "e.vcidx", tmp_path / "f.vcidx")
        # everything removed: an empty handle that accepts records and an index again
        assert e.retain(np.zeros(len(e), dtype=np.uint32))[0] == 0 and len(e) == 0 and _no_index(vc, e, codes[:1])
        n_kept, ids = e.retain(np.zeros(0, dtype=np.uint32))                 # N == 0
        assert n_kept == 0 and len(ids) == 0
        e.add_codes(codes[keep])
        e.build_index()
        a, b = e.search_knn(codes[:8], 10, mode=vc.MODE_MIH_EXACT), f.search_knn(codes[:8], 10, mode=vc.MODE_MIH_EXACT)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert _same_codes(e, f, tmp_path)
    with vc.Engine(bits, capacity=len(codes), n_tables=m) as e, vc.Engine(bits, capacity=len(codes), n_tables=m) as f:
        e.add_codes(codes)                                    # no index before: none after
        assert e.retain(keep.astype(np.uint32))[0] == keep.sum() and _no_index(vc, e, codes[:1])
        f.add_codes(codes[keep])
        assert _same_codes(e, f, tmp_path)
        a, b = e.search_knn(codes[:8], 10), f.search_knn(codes[:8], 10)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_errors_leave_everything_untouched(vc, monkeypatch):
    """10. every VC_ERR_INVALID case leaves the size, a sentinel-filled new_ids and n_kept untouched; N == 0 is VC_OK"""
    import ctypes as C
    _clean_env(monkeypatch)
    bits, m = 64, 4
    codes = R.db_codes(bits, m, 0, 500)
    L = vc.load_library()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with vc.Engine(bits, capacity=len(codes), n_tables=m) as e:
        kept = C.c_uint64(12345)
        assert L.vc_retain(e._h, None, 0, None, C.byref(kept)) == vc.VC_OK and kept.value == 0       # N == 0: nothing read or written
        assert L.vc_retain_dev(e._h, None, 0, None, None, None) == vc.VC_OK
        e.add_codes(codes)
        e.build_index()
        n = len(codes)
        sel = np.ones(n, dtype=np.uint32)
        sel[::2] = 0
        sentinel = np.full(2 * n, 0xABCDEF01, dtype=np.uint32)
        kept = C.c_uint64(12345)
        calls = (
            lambda: L.vc_retain(None, p(sel), 0, p(sentinel), C.byref(kept)),
            lambda: L.vc_retain(e._h, None, 0, p(sentinel), C.byref(kept)),
            lambda: L.vc_retain(e._h, p(sel), 2, p(sentinel), C.byref(kept)),
            lambda: L.vc_retain(e._h, p(sel), 0xFFFFFFFF, p(sentinel), C.byref(kept)),
            lambda: L.vc_retain(e._h, p(sentinel), 0, p(sentinel[n - 1:]), C.byref(kept)),      # new_ids overlaps sel by one word
            lambda: L.vc_retain(e._h, p(sentinel[1:]), 0, p(sentinel), C.byref(kept)),
            lambda: L.vc_retain_dev(None, p(sel), 0, None, C.byref(kept), None),
            lambda: L.vc_retain_dev(e._h, None, 1, None, C.byref(kept), None),
            lambda: L.vc_retain_dev(e._h, p(sel), 2, None, C.byref(kept), None),
            lambda: L.vc_retain_dev(e._h, p(sentinel), 0, p(sentinel[n - 1:]), C.byref(kept), None),
        )
        for i, call in enumerate(calls):
            assert call() == vc.VC_ERR_INVALID, i
            assert len(e) == n and kept.value == 12345 and np.all(sentinel == 0xABCDEF01), i
        rows, cnt = e.search_knn(codes[:4], 5, mode=vc.MODE_MIH_EXACT)                           # the index is still there
        assert np.all(cnt == 5)
        with pytest.raises(vc.VcError):
            e.retain(sel[:-1])


# ---------------------------------------------------------------- 11. host and device form
@pytest.mark.parametrize("stream_kind", ["null", "own", "torch"])
def test_device_form_equals_host_form(vc, monkeypatch, capfd, tmp_path, stream_kind):
    """11. vc_retain_dev on the null stream, on VC_STREAM_OWN and on a non-default torch stream: the result of vc_retain"""
    import torch
    _clean_env(monkeypatch)
    bits, m = 64, 2
    codes, keys = R.db_codes(bits, m, 300, 20000), R.db_keys(bits, m, 300, 20000)
    keep = R.mask("whole_buckets", keys, bits, m) & R.mask("sparse", keys, bits, m)
    K, n = int(keep.sum()), len(codes)
    with vc.Engine(bits, capacity=n, n_tables=m) as d, vc.Engine(bits, capacity=n, n_tables=m) as h:
        for e in (d, h):
            e.add_codes(codes)
            e.build_index()
        kept_h, ids_h = h.retain(keep.astype(np.uint32))
        side = torch.cuda.Stream() if stream_kind == "torch" else None
        stream = {"null": None, "own": vc.STREAM_OWN, "torch": side.cuda_stream if side else None}[stream_kind]
        with torch.cuda.stream(side) if side else torch.cuda.stream(torch.cuda.current_stream()):
            d_sel = torch.from_numpy(keep.astype(np.int32)).cuda()
            d_map = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        capfd.readouterr()
        kept_d = d.retain_dev(d_sel.data_ptr(), d_new_ids=d_map.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        assert [ln[:3] for ln in _retain_lines(capfd.readouterr().err)] == [(K, n - K, "filter")]
        assert kept_d == kept_h == K == len(d) == len(h)
        assert np.array_equal(d_map.cpu().numpy().view(np.uint32), ids_h) and np.array_equal(ids_h, R.new_ids_model(keep, 0))
        assert _same_codes(d, h, tmp_path)
        _compare_views(d, h, bits, m, keys[keep], _watched_keys(bits, m, keys), 0, stream_kind)
        a, b = d.search_knn(codes[:8], 10, mode=vc.MODE_MIH_EXACT, with_stats=True), h.search_knn(codes[:8], 10, mode=vc.MODE_MIH_EXACT, with_stats=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and _host_stats(a[2]) == _host_stats(b[2])
