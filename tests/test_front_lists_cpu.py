"""The numpy definition of the step's edge lists (tests/front_lists_ref.py) against plain loops, and the host side of
ddp_front_lists: header, binding and limits agree."""
import os
import re

import numpy as np
import pytest

import front_lists_ref as FR
from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import build as B

SMALL = {k: FR.CASES[k] for k in ("b1_small", "b1_single_atom_no_bonds", "b2_one_sample_empty", "b2_all_empty")}
SMALL["b2_ll_short"] = dict(seed=12, nl=[7, 5], nr=[3, 4], na=[10, 12], nt=[1, 1], cut=[9.0, 12.0], ll_short=25)
SMALL["b2_tiny_cap"] = dict(seed=11, nl=[7, 5], nr=[3, 9], na=[20, 31], nt=[2, 1], cut=[9.0, 12.0], ll_nb=4, tor_nb=3, la_per_atom=2)


def _val(out, n):
    a = np.full(n, -1, dtype=np.int64)
    a[out.idx] = out.val
    return a


@pytest.mark.parametrize("name", list(SMALL))
def test_definition_against_loops(name):
    c = FR.case(**SMALL[name])
    d, n = FR.front_lists_def(c), FR.sizes(c)
    lists = {"ll": (c.lpos, c.ptr_l, c.lpos, c.ptr_l, c.r_lig, c.ll_nb, True, None, c.Eb, c.cap_ll, "ll1", "ll0"),
             "lr": (c.rpos, c.ptr_r, c.lpos, c.ptr_l, c.r_cross, 10000, False, c.cut, 0, c.cap_lr, "lr0", "lr1"),
             "la": (c.apos, c.ptr_a, c.lpos, c.ptr_l, c.r_lig, 10000, False, None, 0, c.cap_la, "la0", "la1")}
    if c.T:
        lists["tor"] = (c.lpos, c.ptr_l, c.tpos, c.ptr_t, c.r_lig, c.tor_nb, False, None, 0, c.cap_tor, "tor_q", "tor_x")
    full = {}
    for key, (x, xp, y, yp, r, cap_nb, drop, div, base, cap, qn, xn) in lists.items():
        q, p = FR.naive_radius(x, xp, y, yp, r, cap_nb, drop, div)
        assert int(d[f"cnt.{key}"].val[0]) == base + q.shape[0]
        kept = min(base + q.shape[0], cap)
        qa, xa = _val(d[qn], n[qn]), _val(d[xn], n[xn])
        assert np.array_equal(qa[base:kept], q[:kept - base]) and np.array_equal(xa[base:kept], p[:kept - base])
        assert (qa[kept:] == -1).all() and (xa[kept:] == -1).all()
        if base:
            qa[:base], xa[:base] = c.bond1, c.bond0
        full[key] = (qa[:kept], xa[:kept], kept)
    q, p = FR.naive_radius(c.lpos, c.ptr_l, c.apos, c.ptr_a, c.r_lig, 10000)
    touched = np.bincount(q, minlength=c.Na) if c.Na else np.zeros(0, dtype=np.int64)
    assert np.array_equal(_val(d["touched"], n["touched"])[:c.Na], touched)
    near = np.nonzero(touched)[0]
    assert int(d["cnt.near"].val[0]) == near.shape[0] and np.array_equal(_val(d["near_rows"], n["near_rows"])[:near.shape[0]], near)
    assert int(d["overflow"].val[0]) == int(int(d["cnt.la"].val[0]) > c.cap_la)
    # the views by plain loops: c_x by the point (ll: by ll0), so_x = c_x by its source payload
    for view, key, (by, pay), nk in (("c_ll", "ll", (1, 0), c.Nl), ("c_la", "la", (1, 0), c.Na), ("c_lr", "lr", (1, 0), c.Nr)):
        qa, xa, kept = full[key]
        arrs = (qa, xa)
        rp, perm = FR.naive_group(arrs[by], kept, nk)
        assert np.array_equal(_val(d[f"{view}.rp"], n[f"{view}.rp"])[:nk + 1], rp)
        assert np.array_equal(_val(d[f"{view}.perm"], n[f"{view}.perm"])[:kept], perm)
        assert np.array_equal(_val(d[f"{view}.key"], n[f"{view}.key"])[:kept], arrs[by][perm])
        assert np.array_equal(_val(d[f"{view}.o0"], n[f"{view}.o0"])[:kept], arrs[pay][perm])
        so = "so" + view[1:]
        src = arrs[pay][perm]
        rp2, perm2 = FR.naive_group(src, kept, c.Nl)
        assert np.array_equal(_val(d[f"{so}.rp"], n[f"{so}.rp"])[:c.Nl + 1], rp2)
        assert np.array_equal(_val(d[f"{so}.perm"], n[f"{so}.perm"])[:kept], perm2)
        assert np.array_equal(_val(d[f"{so}.key"], n[f"{so}.key"])[:kept], src[perm2])
        assert np.array_equal(_val(d[f"{so}.o0"], n[f"{so}.o0"])[:kept], arrs[by][perm][perm2])
        assert np.array_equal(_val(d[f"{so}.o1"], n[f"{so}.o1"])[:kept], perm[perm2])
        if key != "ll":      # regrouping a point-grouped query-major list by query restores the list
            assert np.array_equal(perm[perm2], np.arange(kept))
    for rp_name, key, nk in (("rp_lr", "lr", c.Nl), ("rp_la", "la", c.Nl)) + ((("rp_tor", "tor", c.T),) if c.T else ()):
        qa, _, kept = full[key]
        assert np.array_equal(_val(d[rp_name], n[rp_name])[:nk + 1], FR.naive_group(qa, kept, nk)[0])


def test_cases_cover_the_boundaries():
    cs = [FR.case(**a) for a in FR.CASES.values()]
    assert {c.B for c in cs} >= {1, 2, 5}
    assert {x for c in cs for x in c.nl} >= {1, 3, 34, 40} and {x for c in cs for x in c.nr} >= {1, 63, 64, 65, 139}
    assert {x for c in cs for x in c.na} >= {64, 65, 1111}
    assert any(c.Eb == 0 for c in cs) and any(c.Eb > 0 for c in cs)
    assert any(c.cut is not None and len(set(c.cut.tolist())) > 1 for c in cs)
    d = {k: FR.front_lists_def(FR.case(**a)) for k, a in FR.CASES.items()}
    assert int(d["b2_la_overflow"]["overflow"].val[0]) == 1 and int(d["b2_cap_binds"]["overflow"].val[0]) == 0
    assert int(d["b3_ll_capacity"]["cnt.ll"].val[0]) > FR.case(**FR.CASES["b3_ll_capacity"]).cap_ll + 100      # the list is cut short
    assert all(int(d["b2_all_empty"][f"cnt.{k}"].val[0]) == 0 for k in ("ll", "lr", "la", "near"))
    assert (d["b2_all_empty"]["c_la.rp"].val == 0).all()
    c = FR.case(**FR.CASES["b2_cap_binds"])        # 40 packed atoms: 33 matches are met, the self pair is among them for q < 33
    cnt = np.bincount(d["b2_cap_binds"]["ll1"].val - 0, minlength=c.Nl)[c.ptr_l[1]:c.ptr_l[2]]
    assert cnt[:33].tolist() == [32] * 33 and cnt[33:].tolist() == [33] * 7


def test_header_binding_and_limits():
    with open(os.path.join(B.ROOT, "include", "ddp_hip.h")) as f:
        header = f.read()
    assert "#define DDP_ABI_VERSION 17" in header and "ddp_front_lists" in L.EXPORTS and "ddp_front_lists.hip" in B.SOURCES
    assert any(h.endswith("ddp_radius_math.h") for h in B.HEADERS)
    for name in ("LIG", "REC", "ATOM", "BONDS"):
        assert int(re.search(rf"#define DDP_FRONT_MAX_{name} (\d+)", header).group(1)) == getattr(L, f"DDP_FRONT_MAX_{name}")
    body = re.search(r"typedef struct \{([^}]*)\} ddp_front_lists_t;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].strip("*") for n in names]
    assert names == [f[0] for f in L.FrontLists._fields_]
    vbody = re.search(r"typedef struct \{([^}]*)\} ddp_front_view_t;", header).group(1)
    assert re.findall(r"\*\s*(\w+);", vbody) == [f[0] for f in L.FrontView._fields_]
