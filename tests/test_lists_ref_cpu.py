"""tests/lists_ref.py against naive Python loops at tiny sizes, and the case tables of tests/test_gpu_list_seams.py
(tests/list_seam_cases.py) for being well formed - no device."""
import numpy as np
import pytest

import list_seam_cases as T
import lists_ref as R


def _same(out, want):
    """`want`: {position: value}; the definition's index set is exactly its keys."""
    idx = np.asarray(out.idx)
    assert len(set(idx.tolist())) == idx.shape[0]
    assert dict(zip(idx.tolist(), np.asarray(out.val).tolist())) == want


@pytest.mark.parametrize("mode", T.SCAN_MODES)
@pytest.mark.parametrize("n,n_dev,base", [(0, None, 3), (1, None, 0), (7, 5, 11), (40, 44, 0), (9, -3, 2)])
def test_scan_definition(mode, n, n_dev, base):
    c = T.scan_case(5, mode, n, base=base)
    got = R.scan(n, n_dev, c.get("flag"), c.get("val"), c.get("rowptr"), base)
    cnt = n if n_dev is None else min(max(n_dev, 0), n)
    run, excl, lst = base, {}, {}
    for i in range(cnt):
        excl[i] = run
        v = 1
        if "val" in c:
            v = int(c["val"][i])
        elif "rowptr" in c:
            v = int(c["rowptr"][i + 1] - c["rowptr"][i])
        if "flag" in c and c["flag"][i] == 0:
            v = 0
        if v and "val" not in c and "rowptr" not in c:
            lst[run] = i
        run += v
    _same(got["excl2"], dict(excl))
    excl[cnt] = run
    _same(got["excl"], excl)
    _same(got["total"], {0: run})
    if "val" not in c and "rowptr" not in c:
        _same(got["list"], lst)
    else:
        assert "list" not in got


def test_mark_definition():
    idx = np.array([3, 3, 0, 7, 3, 9])
    _same(R.mark(6, 4, idx)["mask"], {3: 1, 0: 1, 7: 1})
    _same(R.mark(6, None, None)["mask"], {i: 1 for i in range(6)})
    _same(R.mark(6, -1, idx)["mask"], {})


def test_rowcopy_definition():
    rng = np.random.default_rng(0)
    lens = np.array([2, 0, 5, 1, 3, 0, 4])
    keep = np.array([1, 1, 0, 2, 0, 1, 1])
    old = np.concatenate([[0], np.cumsum(lens)])
    new = np.concatenate([[0], np.cumsum(lens * (keep != 0))])
    ins = [rng.integers(0, 99, 15), rng.integers(0, 99, 15)]
    got = R.rowcopy(7, keep, old, new, ins)["outs"]
    for k in range(2):
        want = {}
        for r in range(7):
            if keep[r]:
                for a in range(lens[r]):
                    want[int(new[r] + a)] = int(ins[k][old[r] + a])
        _same(got[k], want)


@pytest.mark.parametrize("form", T.SELECT_FORMS)
@pytest.mark.parametrize("n_dev", [None, 25, 0, 99])
def test_select_definition(form, n_dev):
    c = T.select_case(3, 40, n_dev, "some", form, 2, pay_add=[0, 5])
    got = R.select(40, n_dev, c["mask_a"], c["idx_a"], c["mask_b"], c["idx_b"], c["pays"], c["pay_add"])
    cnt = 40 if n_dev is None else min(n_dev, 40)
    kept = []
    for i in range(cnt):
        f = False
        if c["mask_a"] is not None:
            f = f or c["mask_a"][c["idx_a"][i] if c["idx_a"] is not None else i] != 0
        if c["mask_b"] is not None:
            f = f or c["mask_b"][c["idx_b"][i] if c["idx_b"] is not None else i] != 0
        if f:
            kept.append(i)
    _same(got["out_idx"], dict(enumerate(kept)))
    _same(got["outs"][1], {j: int(c["pays"][1][i]) + 5 for j, i in enumerate(kept)})
    _same(got["total"], {0: len(kept)})


def test_gather_rows_definition():
    x = np.arange(7 * 6).reshape(7, 6) - 20
    idx = np.array([5, 5, 0, 6])
    got = R.gather_rows(x, idx, 4, 3, ncols=4, ldo=9)["out"]
    _same(got, {i * 9 + c: int(x[idx[i], c]) for i in range(3) for c in range(4)})


@pytest.mark.parametrize("with_rowptr", [False, True])
def test_clean_pair_maps_definition(with_rowptr):
    c = T.clean_case(1, 3, 6, 13, with_rowptr)
    got = R.clean_pair_maps(c["touched"], c["recv"], c["src"], c["E"], 13, 3, 6, c["rowptr"])
    want = {}
    for p in range(39):
        r = int(c["recv"][p])
        if c["touched"][r] or c["touched"][c["src"][p]]:
            want[p] = p
        elif with_rowptr:
            want[p] = 39 + int(c["rowptr"][r % 6]) + p - int(c["rowptr"][r])
        else:
            want[p] = 39 + p % 13
    _same(got["rowmap"], want)
    rows = {}
    for a0 in range(6):
        g = next((b for b in range(3) if c["touched"][b * 6 + a0] == 0), 0)
        rows[a0] = g * 6 + a0
    _same(got["rows_v"], rows)
    assert any(v == i for i, v in rows.items()) and any(v >= 6 for v in rows.values())


@pytest.mark.parametrize("how", ["moved", "ulp", "zero", "flag"])
@pytest.mark.parametrize("n_a,a_too,ref_list", [(5, False, True), (9, True, True), (9, True, False)])
def test_flex_mark_definition(how, n_a, a_too, ref_list):
    c = T.flex_case(2, 3, n_a, 9, 13, a_too, ref_list, how)
    got = R.flex_mark(c["a"], c["b"], 39, 13, n_a, 9, pos=c["pos"], flag=c["flag"], a_too=a_too, ref_list=ref_list)["mark"]
    off = c["off"].reshape(-1)              # how the case was made: which atom of which sample moved / is flagged
    assert off.any()
    want = {i: 1 for i in range(n_a)}
    for e in range(13, 39):
        s = e // 13
        ai, bi = int(c["a"][e]), int(c["b"][e])
        if off[bi] or (a_too and off[ai]):
            want[ai] = 1
        if ref_list:
            l = e - 13 * s
            if off[int(c["b"][l]) + s * 9]:
                want[int(c["a"][l]) + s * n_a] = 1
    _same(got, want)


def test_flex_mark_definition_compares_bits():
    """-0.0 against +0.0 and a one-ulp step are differences; a NaN equals its own copy."""
    nan = 0x7fc00123
    pos = np.array([[0, 5, 7], [nan, 1, 2], [T.NEG_ZERO, 5, 7], [nan, 1, 2]])       # two samples of two atoms
    a, b = np.array([0, 1, 2, 3]), np.array([0, 1, 2, 3])
    _same(R.flex_mark(a, b, 4, 2, 2, 2, pos=pos)["mark"], {0: 1, 1: 1, 2: 1})
    pos[2, 0], pos[3, 2] = 0, 3
    _same(R.flex_mark(a, b, 4, 2, 2, 2, pos=pos)["mark"], {0: 1, 1: 1, 3: 1})


def test_fallback_rowmap_definition():
    c = T.fallback_case(5, 3, 6, 30)
    got = R.fallback_rowmap(c["mark"], c["recv"], c["old_rowptr"], c["new_rowptr"], 30, 6)["rowmap"]
    want = {}
    for p in range(30):
        r = int(c["recv"][p])
        t = r if c["mark"][r] else r % 6
        want[p] = int(c["new_rowptr"][t]) + p - int(c["old_rowptr"][r])
    _same(got, want)


@pytest.mark.parametrize("n_dev,key_map", [(None, False), (25, True), (0, False)])
def test_group_by_key_definition(n_dev, key_map):
    c = T.group_case(1, 40, n_dev, 7, n_pay=2, key_map=key_map)
    got = R.group_by_key(c["key"], 40, n_dev, 7, c["pays"], c["key_map"])
    cnt = 40 if n_dev is None else n_dev
    rows = [[i for i in range(cnt) if c["key"][i] == k] for k in range(7)]
    rp, perm = {0: 0}, []
    for k in range(7):
        perm += rows[k]
        rp[k + 1] = len(perm)
    _same(got["rowptr"], rp)
    _same(got["perm"], dict(enumerate(perm)))
    km = c["key_map"] if key_map else np.arange(7)
    _same(got["out_key"], {p: int(km[c["key"][i]]) for p, i in enumerate(perm)})
    _same(got["outs"][1], {p: int(c["pays"][1][i]) for p, i in enumerate(perm)})
    assert got["scratch"].val is None and got["scratch"].idx.shape[0] == 7 + cnt
    only = R.group_by_key(c["key"], 40, n_dev, 7, perm=False)
    assert set(only) == {"rowptr", "scratch"} and only["scratch"].idx.shape[0] == 7


# ------------------------------------------------------------------------------------------------ the GPU file's case tables
I32 = 2 ** 31


def _in_i32(*arrays):
    for a in arrays:
        if a is not None:
            a = np.asarray(a)
            assert a.size == 0 or (int(a.min()) >= -I32 and int(a.max()) < I32)


@pytest.mark.parametrize("table,form", [("sweep", "small"), ("sweep", "general"), ("large", "general"), ("scalar", "small"), ("scalar", "general")])
def test_scan_tables(table, form):
    groups = {"sweep": T.scan_sweep, "scalar": T.scan_scalar}[table](form) if table != "large" else T.scan_large()
    assert len(groups) > 1 and all(len(g) == T.MAX_JOBS for g in groups[:-1]) and 0 < len(groups[-1]) <= T.MAX_JOBS
    seen = set()
    for g in groups:
        assert T.scan_form(g) == form                           # the kernel's rule, over the jobs of one launch
        for c in g:
            assert c["cap"] <= 100003 + 37 and (c["n_dev"] is None or -I32 <= c["n_dev"] < I32)
            assert c["n"] == R.count(c["cap"], c["n_dev"])
            m = max(c["cap"], 1)
            for k in ("flag", "val"):
                assert k not in c or c[k].shape[0] == m
            assert "rowptr" not in c or (c["rowptr"].shape[0] == m + 1 and (np.diff(c["rowptr"]) >= 0).all())
            out = R.scan(c["cap"], c["n_dev"], c.get("flag"), c.get("val"), c.get("rowptr"), c["base"])
            assert 0 <= int(out["total"].val[0]) < I32           # totals below 2^31
            assert ("list" in out) == ("list" in T.SCAN_OUTPUTS[c["mode"]])
            if "list" in out and out["list"].idx.shape[0]:
                assert int(out["list"].idx.max()) < c["base"] + m
            assert c["odd"] is None or c["odd"] in T.SCAN_ODD[c["mode"]]
            seen.add((c["mode"], c["odd"] is not None))
    assert {m for m, _ in seen} == set(T.SCAN_MODES)            # every mode in this form ...
    if table == "scalar":
        assert all((m, True) in seen for m in T.SCAN_MODES)     # ... and on the scalar path
        assert {(c["mode"], c["odd"]) for g in groups for c in g} >= {(m, o) for m in T.SCAN_MODES for o in T.SCAN_ODD[m]}
    if table == "sweep":
        ns = {(c["mode"], c["n"]) for g in groups for c in g}
        assert all((m, n) in ns for m in T.SCAN_MODES for n in T.SCAN_SIZES)
        kinds = {("none" if c["n_dev"] is None else "neg" if c["n_dev"] < 0 else "over" if c["n_dev"] > c["cap"] else
                  "slack" if c["n_dev"] < c["cap"] else "eq") for g in groups for c in g}
        assert kinds == {"none", "neg", "over", "slack", "eq"}
        flat = [c for g in groups for c in g]
        assert any(a["n"] > 0 and b["n"] == 0 and c["n"] > 0 for a, b, c in zip(flat, flat[1:], flat[2:]))
        S = T.scan_segment(4097)
        assert S == 512 and T.scan_segment(4096) == 256 and T.scan_segment(49152) == 3072 and T.scan_segment(53248) == 3328


def test_select_tables():
    sweep = T.select_sweep()
    assert {(c["cap"], c["flags"]) for c in sweep} >= {(n, f) for n in T.SELECT_SIZES for f in T.SELECT_FLAGS}
    assert {c["form"] for c in sweep} == set(T.SELECT_FORMS)
    assert any(not c["out_idx"] for c in sweep) and any(c["drop_out"] for c in sweep) and any(c["pay_add"] and any(c["pay_add"]) for c in sweep)
    assert {len(c["pays"]) for c in sweep} >= {1, 2, 3, 4}
    twelve, thirteen, empties = T.select_tables()
    assert len(twelve) == 12 and len({c["cap"] for c in twelve}) == 12 and all(c["cap"] > 0 for c in twelve)
    assert len(thirteen) == 13 and [c["cap"] == 0 for c in empties] == [True, False, True, False, True]
    assert len({c["total0"] for c in empties if c["cap"] == 0}) == 3
    for c in sweep + twelve + thirteen + empties:
        m = max(c["cap"], 1)
        for mk, ik in (("mask_a", "idx_a"), ("mask_b", "idx_b")):
            if c[mk] is None:
                assert c[ik] is None
            elif c[ik] is None:
                assert c[mk].shape[0] == m
            else:
                assert c[ik].shape[0] == m and 0 <= c[ik].min() and c[ik].max() < c[mk].shape[0]
        assert c["mask_a"] is not None or c["mask_b"] is not None
        assert all(p.shape[0] == m for p in c["pays"]) and all(k < len(c["pays"]) for k in c["drop_out"])
        out = R.select(c["cap"], c["n_dev"], c["mask_a"], c["idx_a"], c["mask_b"], c["idx_b"], c["pays"], c["pay_add"])
        _in_i32(*[o.val for o in out["outs"]])
        k, n = int(out["total"].val[0]), R.count(c["cap"], c["n_dev"])
        want = {"all": n, "none": 0, "last": int(n == c["cap"] and n > 0), "block_first": -(-n // 2048)}.get(c["flags"])
        assert want is None or k == want
        assert c["flags"] != "some" or n < 60 or 0 < k < n


def test_mark_and_rowcopy_tables():
    for call in T.mark_calls():
        assert len(call) == 3 and call[1]["n"] == 0 and call[0]["n"] > 0 and call[2]["n"] > 0
        for j in call:
            if j["idx"] is not None:
                assert j["idx"].shape[0] == max(j["n"], 1) and 0 <= j["idx"].min() and j["idx"].max() < T.MARK_MASK
            assert j["n"] <= T.MARK_MASK
    calls = T.rowcopy_calls()
    assert {j["n_rows"] for c in calls for j in c} == {0, 1, 3, 4, 5, 129} and {len(j["ins"]) for c in calls for j in c} == {1, 2, 3}
    for call in calls:
        assert len(call) <= T.MAX_JOBS and any(a["n_rows"] and b["n_rows"] == 0 and c["n_rows"] for a, b, c in zip(call, call[1:], call[2:]))
        for j in call:
            assert j["old_rowptr"].shape[0] == j["n_rows"] + 1 and j["old_rowptr"][-1] == j["n_edges"]
            assert set(np.diff(j["old_rowptr"]).tolist()) <= set(T.ROW_LENGTHS)
            assert all(x.shape[0] == max(j["n_edges"], 1) for x in j["ins"])


def test_gather_tables():
    cases = T.gather_cases()
    assert {(c["ncols"], c["n"]) for c in cases} == {(nc, n) for nc in (1, 63, 64, 65, 130) for n in (1, 3, 4, 5, 301)}
    assert {("none" if c["n_dev"] is None else "zero" if c["n_dev"] == 0 else "below" if c["n_dev"] < c["n"] else "above") for c in cases} == \
        {"none", "zero", "below", "above"}
    for c in cases:
        assert c["ldx"] == c["ncols"] + 3 and c["ldo"] == c["ncols"] + 5 and c["x"].shape == (c["rows"], c["ldx"])
        assert 0 <= c["idx"].min() and c["idx"].max() < c["rows"] and (c["n"] < 3 or len(set(c["idx"].tolist())) < c["n"])
        _in_i32(c["x"])
    x = np.concatenate([c["x"].reshape(-1) for c in cases]).astype(np.int32).view(np.float32)
    assert np.isnan(x).any() and (np.signbit(x) & (x == 0)).any()


def test_clean_pair_tables():
    cases = T.clean_cases()
    assert any(c["E"] < c["n0"] and c["B"] == 2 for c in cases) and {256, 257} <= {c["E"] for c in cases} and any(c["B"] == 1 for c in cases)
    for c in cases:
        B, n0, e0, E = c["B"], c["n0"], c["e0"], c["E"]
        assert E == e0 * B < I32 and c["recv"].shape == c["src"].shape == (E,) and c["touched"].shape == (B * n0,)
        assert (np.diff(c["recv"]) >= 0).all()
        for s in range(B):                                          # every sample keeps e0 edges, ends inside the sample
            for x in (c["recv"], c["src"]):
                assert (x[s * e0:(s + 1) * e0] // n0 == s).all()
        t = c["touched"].reshape(B, n0)
        assert (t != 0).all(0).any()                                 # an atom touched in every sample
        lens = np.bincount(c["recv"], minlength=B * n0).reshape(B, n0)
        if c["rowptr"] is None:
            assert (lens == lens[0]).all() and (c["src"].reshape(B, e0) % n0 == c["src"][:e0]).all()
        else:
            assert (np.diff(c["rowptr"]) == lens.reshape(-1)).all()
            assert (lens[t == 0] == np.broadcast_to(lens[0], lens.shape)[t == 0]).all()          # untouched: the copy's row length
            assert B == 1 or (lens[t != 0] != np.broadcast_to(lens[0], lens.shape)[t != 0]).any()
            ref = R.clean_pair_maps(c["touched"], c["recv"], c["src"], E, e0, B, n0, c["rowptr"])["rowmap"].val
            assert ref.min() >= 0 and ref.max() < E + e0
    assert any(c["rowptr"] is not None and c["B"] > 1 and
               (R.clean_pair_maps(c["touched"], c["recv"], c["src"], c["E"], c["e0"], c["B"], c["n0"], c["rowptr"])["rowmap"].val !=
                R.clean_pair_maps(c["touched"], c["recv"], c["src"], c["E"], c["e0"], c["B"], c["n0"])["rowmap"].val).any() for c in cases)


def test_flex_and_fallback_tables():
    cases = T.flex_cases()
    assert any(c["n_a"] == 23 and c["n_b"] == 57 and not c["a_too"] for c in cases) and any(c["n_edges"] < c["n_a"] for c in cases)
    assert {256, 257, 258} <= {c["n_edges"] for c in cases}
    for c in cases:
        B, e0 = c["B"], c["e0"]
        assert c["n_edges"] == e0 * B < I32 and (not c["a_too"] or c["n_a"] == c["n_b"])
        for s in range(B):
            assert (c["a"][s * e0:(s + 1) * e0] // c["n_a"] == s).all() and (c["b"][s * e0:(s + 1) * e0] // c["n_b"] == s).all()
        if c["pos"] is not None:
            _in_i32(c["pos"])
            p = c["pos"].reshape(B, c["n_b"], 3)
            assert ((p != p[0]).any(2) == c["off"]).all()
            f = p.astype(np.int32).view(np.float32)
            if c["how"] == "zero" and B > 1:                         # differs in bits, equal as floats
                assert c["off"].any() and (f == f[0]).all()
            if c["how"] == "ulp" and B > 1:
                assert c["off"].any() and np.abs(p - p[0]).max() == 1
    for c in T.fallback_cases():
        B, n, E = c["B"], c["n"], c["n_edges"]
        assert c["recv"].shape == (E,) and c["old_rowptr"][-1] == E and c["mark"][:n].all()
        lens = np.diff(c["old_rowptr"]).reshape(B, n)
        m = c["mark"].reshape(B, n) != 0
        assert (lens[~m] == np.broadcast_to(lens[0], lens.shape)[~m]).all()                      # unmarked: the copy's row length
        assert (np.diff(c["new_rowptr"]) == (lens * m).reshape(-1)).all()
        out = R.fallback_rowmap(c["mark"], c["recv"], c["old_rowptr"], c["new_rowptr"], E, n)["rowmap"].val
        assert out.min() >= 0 and out.max() < c["new_rowptr"][-1]
    assert {c["n_edges"] for c in T.fallback_cases()} >= {1, 255, 257}


def test_group_tables():
    calls = T.group_calls()
    assert {c["n_keys"] for _, jobs in calls for c in jobs} >= {1, 255, 256, 257, 49152, 49153, 60000}
    for form, jobs in calls:
        assert T.group_form(jobs) == form and len(jobs) == T.MAX_JOBS
        assert any(c["perm"] for c in jobs) and any(not c["perm"] for c in jobs) and any(c["odd_rowptr"] for c in jobs)
        assert any(a["n_items"] and b["n_items"] == 0 and c["n_items"] for a, b, c in zip(jobs, jobs[1:], jobs[2:]))
        for c in jobs:
            assert c["n_keys"] + c["n_items"] <= 100003 and c["key"].shape[0] == max(c["n_items"], 1)
            assert 0 <= c["key"].min() and c["key"].max() < c["n_keys"]
            assert all(k < len(c["pays"]) for k in c["drop_out"])
    small = calls[0][1]
    assert {R.count(c["n_items"], c["n_dev"]) for c in small} >= {255, 256, 257, 0}
    rows = np.bincount(small[4]["key"], minlength=5)
    assert rows.tolist() == [0, 65, 130, 200, 0] and np.bincount(small[6]["key"]).max() == 3000
