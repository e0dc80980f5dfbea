"""diffdock_pocket_amd/minimize_flex.py without a device: the sc_pairs table against a mask written out by hand; the PyTorch energy and
both gradients against the NumPy restatement of tests/flexmin_ref.py and against its central differences; the side-chain direction
against the restatement's derivative along a rotation; the invariants of a 20-iteration run on the small flexible complex; equality
with PoseMinimizer without side-chain bonds; the C entry's declaration, export, struct and launch-free guards; the flags and run_csv."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import flexmin_ref as F
from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import minimize as M
from diffdock_pocket_amd import minimize_flex as MF
from diffdock_pocket_amd import outputs as O
from diffdock_pocket_amd import refine as R
from diffdock_pocket_amd.batch import Store
from diffdock_pocket_amd.sampler import apply_sidechain_torsions
from diffdock_pocket_amd.synthetic import make_3dpf_complex
from test_minimize_cpu import bits32
from test_scoring_cpu import CFG, CSV, ROOT, _rows, _run

_CACHE = {}


# ---------------------------------------------------------------------------------------------- shared helpers
def torch_case(c):
    """The tensors of a flexmin_ref.random_case, in the argument order of minimize_flex.energy_flex_torch up to sc_pairs."""
    t = {k: torch.from_numpy(c[k]) for k in ("x", "y", "x0", "y0", "lig_r", "lig_f", "rec_r", "rec_f", "mov", "sc_pairs", "edge", "sub", "mapping")}
    t["pairs"] = None if c["pairs"] is None else torch.from_numpy(c["pairs"])
    return t


def torch_energy(c, x=None, y=None):
    t = torch_case(c)
    return MF.energy_flex_torch(t["x"] if x is None else x, t["y"] if y is None else y, t["x0"], t["y0"], t["lig_r"], t["lig_f"], t["rec_r"],
                                t["rec_f"], t["pairs"], t["mov"], t["sc_pairs"], CFG, c["k"], c["k_sc"])


def ref_E(c, x, y):
    return F.energy(x, y, c["x0"], c["y0"], c["lig_r"], c["lig_f"], c["rec_r"], c["rec_f"], c["pairs"], c["mov"], c["sc_pairs"], c["k"],
                    c["k_sc"])["energy"][:, 5]


def small_flexible_case():
    """(graph, poses [3, 12, 3], atom_pos [3, m, 3]) of the small flexible synthetic complex, the side chains of every sample perturbed
    by chi noise N(0, 0.5 rad) of torch.Generator().manual_seed(11), the ligand by N(0, 0.3 A) per atom; built once.  The synthetic
    graph draws its atom features, the elements among them, at random: with the default seed 0 all four moving atoms come out untyped
    and take part in nothing; seed 2 types two of them (and 14 receptor atoms in all)."""
    if "small" not in _CACHE:
        g = make_3dpf_complex(seed=2, flexible_sidechains=True, n_lig=12, n_rec=8)
        gen = torch.Generator().manual_seed(11)
        lig = (g["ligand"].pos.float()[None] + 0.3 * torch.randn(3, 12, 3, generator=gen)).contiguous()
        fr = g["flexResidues"]
        chi = 0.5 * torch.randn(3, fr.edge_idx.shape[0], generator=gen)
        apos = apply_sidechain_torsions(g["atom"].pos.float()[None].repeat(3, 1, 1), fr.edge_idx, fr.subcomponents, fr.subcomponentsMapping, chi)
        _CACHE["small"] = (g, lig, apos.contiguous())
    return _CACHE["small"]


# ---------------------------------------------------------------------------------------------- 1. the pair table
def test_sc_pairs_of_a_hand_built_receptor():
    """A chain 0 - 1 - ... - 9 with two nested side-chain bonds: bond 0 = (3, 2) turns atoms 4 .. 9, bond 1 = (6, 5) turns 7 .. 9.  A
    pair counts iff it is more than 3 bonds apart and one bond's subcomponent holds exactly one of the two; rows of the moving atoms
    4 .. 9, written out by hand."""
    m = 10
    nbrs = [[b for b in (a - 1, a + 1) if 0 <= b < m] for a in range(m)]
    sub, mapping = [4, 5, 6, 7, 8, 9, 7, 8, 9], [[0, 6], [6, 9]]
    mask = MF.sidechain_rotate_mask(m, sub, mapping)
    assert mask.astype(int).tolist() == [[0, 0, 0, 0, 1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0, 1, 1, 1]]
    mov = [4, 5, 6, 7, 8, 9]
    got = MF.build_sc_pairs(m, nbrs, mask, mov)
    want = ["1000000011",    # 4: 0 across bond 0 and 4 bonds away; 8, 9 across bond 1
            "1100000001",    # 5
            "1110000000",    # 6: 7, 8, 9 are within 3 bonds
            "1111000000",    # 7
            "1111100000",    # 8
            "1111110000"]    # 9
    assert got.dtype == torch.uint8 and ["".join(str(int(v)) for v in row) for row in got] == want
    # the same rule as the ligand's table, read per moving atom; two static atoms are never a pair
    edge_index = np.array([[a, a + 1] for a in range(m - 1)]).T
    full = R.build_self_pairs(m, edge_index, mask)
    full = full | full.T
    assert torch.equal(full[mov], got) and int(full[:4, :4].sum()) == 0
    # no bond: no pair; an atom without a path to the others is far from all of them
    assert int(MF.build_sc_pairs(m, nbrs, np.zeros((0, m), dtype=bool), mov).sum()) == 0
    lone = MF.build_sc_pairs(m, [[] for _ in range(m)], mask, mov)
    assert ["".join(str(int(v)) for v in row) for row in lone][0] == "1111000111"


def test_tables_of_the_fixture_and_the_host_checks():
    g = make_3dpf_complex(flexible_sidechains=True)
    sc = MF.sidechain_tables(g)
    assert (sc.n_mov, sc.n_sc, int(g["atom"].pos.shape[0])) == (37, 17, 1111) and sc.pairs.shape == (37, 1111)
    assert torch.equal(sc.mov, O.moving_atoms(g)) and bool((sc.mov[1:] > sc.mov[:-1]).all())
    sym = sc.pairs[:, sc.mov]
    assert torch.equal(sym, sym.T) and int(torch.diagonal(sym).sum()) == 0
    assert MF.sidechain_tables(make_3dpf_complex(flexible_sidechains=False)) is None
    e, s, mp = sc.edge_idx, sc.sub, sc.mapping
    MF.check_sidechain_tables(1111, e, s, mp, sc.mov)
    for bad in ((1111, e, s.clone().index_fill_(0, torch.tensor([0]), 1111), mp, None), (1111, e.clone().fill_(-1), s, mp, None),
                (1111, e, s, mp.clone().index_fill_(0, torch.tensor([0]), 10 ** 6), None), (1111, e[:-1], s, mp, None),
                (1111, e, s, mp, sc.mov[1:]), (1111, e, s, mp, sc.mov.flip(0)),
                (1111, e[:1], torch.tensor([5, 5]), torch.tensor([[0, 2]]), None)):
        with pytest.raises(ValueError):
            MF.check_sidechain_tables(*bad)


# ---------------------------------------------------------------------------------------------- 2. energy and gradients
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 0), (3, 5, 40, 4, 1), (2, 37, 130, 37, 17), (1, 4, 60, 5, 17)])
def test_energy_and_both_gradients_match_the_restatement(shape):
    """Within the project's bound form, 256 eps (P + 1) max(1, largest |summand|) (flexmin_ref.bounds); one case with an untyped
    moving atom."""
    for untyped in (False, True):
        c = F.random_case(*shape, seed=11 * sum(shape) + untyped, untyped_moving=untyped)
        e, gx, gy = torch_energy(c)
        ref = c["ref"]
        be, bgx, bgy = F.bounds(ref)
        err = np.abs(e.numpy() - ref["energy"])
        ex, ey = np.abs(gx.numpy() - ref["grad_x"]), np.abs(gy.numpy() - ref["grad_y"])
        print(f"{shape} untyped={untyped}: worst |err| / bound energy {float((err / be).max()):.3e}, dE/dx {float((ex / bgx[:, None, None]).max()):.3e}, "
              f"dE/dy {float((ey / bgy[:, None, None]).max()):.3e}; sc pairs {ref['n_pairs'][:, 2].tolist()}")
        assert (err <= be).all(), err / be
        assert (ex <= bgx[:, None, None]).all() and (ey <= bgy[:, None, None]).all()
        assert e.shape == (shape[0], 6) and gy.shape == (shape[0], shape[3], 3)
        if untyped and shape[3] > 1:        # an untyped moving atom feels the restraint only
            dy = c["y"][:, c["mov"][0]].astype(np.float64) - c["y0"][:, c["mov"][0]].astype(np.float64)
            assert np.allclose(gy[:, 0].numpy(), 2 * c["k_sc"] / shape[3] * dy, rtol=1e-13, atol=0)
    assert shape[3] <= 1 or float(np.abs(ref["energy"][:, 2]).max()) > 0, "the case has no sc term"


def test_gradients_are_the_central_differences_of_the_restatement():
    """fp64 central differences of flexmin_ref.energy with h = 1e-5 A on a case whose pairs keep 1e-3 A from the kinks of the ramps
    and from the cutoff.  Truncation h^2 / 6 |E'''| is about 1e-9 (the Gaussian's third derivative, a few hundred pairs), rounding
    eps |E| / h about 1e-10: the bound is 1e-7 max(1, |g|)."""
    c = F.random_case(1, 5, 30, 4, 2, seed=77, kink_gap=1e-3)
    _, gx, gy = torch_energy(c)
    x, y, h = c["x"].astype(np.float64), c["y"].astype(np.float64), 1e-5
    worst = 0.0
    for i in range(5):
        for k in range(3):
            d = np.zeros_like(x)
            d[0, i, k] = h
            fd = (ref_E(c, x + d, y) - ref_E(c, x - d, y))[0] / (2 * h)
            worst = max(worst, abs(fd - float(gx[0, i, k])) / max(1.0, abs(fd)))
    for r, a in enumerate(c["mov"].tolist()):
        for k in range(3):
            d = np.zeros_like(y)
            d[0, a, k] = h
            fd = (ref_E(c, x, y + d) - ref_E(c, x, y - d))[0] / (2 * h)
            worst = max(worst, abs(fd - float(gy[0, r, k])) / max(1.0, abs(fd)))
    print("worst |finite difference - gradient| / max(1, |g|):", worst, "largest |dE/dy|", float(gy.abs().max()))
    assert worst <= 1e-7 and float(gy.abs().max()) > 1e-3 and float(gx.abs().max()) > 1e-3


def test_the_side_chain_direction_is_the_derivative_along_the_rotation():
    """d_sc[j] sum |a_i|^2 = -dE/d(angle j) at the current pose: against the restatement's central difference along a rotation of
    subcomponent j alone (h = 1e-6 rad, same error reasoning as above; the bound is 1e-6 max(1, |dE/dangle|))."""
    c = F.random_case(2, 5, 30, 6, 3, seed=5, kink_gap=1e-3)
    t = torch_case(c)
    _, _, gy = torch_energy(c)
    d_sc = MF.direction_sc_torch(t["y"], gy, t["mov"], t["edge"], t["sub"], t["mapping"]).numpy()
    x, y, h = c["x"].astype(np.float64), c["y"].astype(np.float64), 1e-6
    worst, largest = 0.0, 0.0
    for j in range(3):
        u, v = c["edge"][j]
        idx = c["sub"][c["mapping"][j, 0]:c["mapping"][j, 1]]
        one = lambda ang: np.stack([F.apply_sidechains(y[s], c["edge"][j:j + 1], idx, [[0, len(idx)]], [ang]) for s in range(2)])
        fd = (ref_E(c, x, one(h)) - ref_E(c, x, one(-h))) / (2 * h)
        for s in range(2):
            axis = (y[s, u] - y[s, v]) / np.linalg.norm(y[s, u] - y[s, v])
            den = (np.cross(axis[None], y[s, idx] - y[s, v]) ** 2).sum()
            worst = max(worst, abs(-d_sc[s, j] * den - fd[s]) / max(1.0, abs(fd[s])))
            largest = max(largest, abs(fd[s]))
    print("worst |d_sc den + dE/dangle| / max(1, |dE/dangle|):", worst, "largest |dE/dangle|", largest)
    assert worst <= 1e-6 and largest > 1e-3
    # a bond whose subcomponent is only its own two atoms has no lever: 0, not NaN
    zero = MF.direction_sc_torch(t["y"], gy, t["mov"], t["edge"][:1], t["edge"][0], torch.tensor([[0, 2]]))
    assert torch.equal(zero, torch.zeros(2, 1, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------- 3. a run
def test_a_20_iteration_run_descends_and_moves_only_the_side_chains():
    g, lig, apos = small_flexible_case()
    mz = MF.FlexPoseMinimizer(g, config=M.MinimizeConfig(iterations=20))
    hist = []
    res = mz.minimize(lig, apos, history=hist)
    h = torch.stack(hist)
    assert h.shape == (21, 3) and bool((h[1:] <= h[:-1]).all()), "the history rises somewhere"
    assert torch.equal(h[0], res.energy_before[:, 5]) and torch.equal(h[-1], res.energy_after[:, 5])
    # iteration by iteration from the same start: the same run, and a rejected iteration keeps x and y bit for bit
    x, y = lig, apos
    step, acc = torch.ones(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32)
    rejected = 0
    for it in range(20):
        x1, y1, step, acc1, e0, e1 = mz.advance(x, y, lig, apos, step, acc, 1)
        for s in range(3):
            if int(acc1[s]) == int(acc[s]):
                rejected += 1
                assert torch.equal(bits32(x1[s]), bits32(x[s])) and torch.equal(bits32(y1[s]), bits32(y[s])) and torch.equal(e0[s], e1[s])
        x, y, acc = x1, y1, acc1
    assert torch.equal(bits32(x), bits32(res.lig_pos)) and torch.equal(bits32(y), bits32(res.atom_pos)) and torch.equal(acc, res.accepted)
    mov = mz.sc.mov
    static = torch.ones(apos.shape[1], dtype=torch.bool)
    static[mov] = False
    assert torch.equal(bits32(res.atom_pos[:, static]), bits32(apos[:, static])), "a static receptor atom changed"
    moved_atoms = int((bits32(res.atom_pos[:, mov]) != bits32(apos[:, mov])).any(-1).sum())
    # bond lengths: the pairs of distance_bonds (the synthetic graph carries random elements, so there are few of them) and, whatever
    # the elements, every pair of atoms closer than 1.9 A in the graph's own positions
    nbrs = MF.receptor_bonds(g)
    ref = g["atom"].pos.double()
    close = torch.nonzero(torch.triu(torch.cdist(ref, ref) < 1.9, 1))
    bonds = torch.cat([torch.tensor([[a, b] for a in range(len(nbrs)) for b in nbrs[a] if a < b], dtype=torch.long).reshape(-1, 2), close])
    assert int(static[bonds].all(1).sum()) < bonds.shape[0], "no bond touches a moving atom"
    length = lambda p: (p[:, bonds[:, 0]].double() - p[:, bonds[:, 1]].double()).norm(dim=-1)
    worst = float((length(res.atom_pos) - length(apos)).abs().max())
    print(f"E {res.energy_before[:, 5].tolist()} -> {res.energy_after[:, 5].tolist()}; accepted {res.accepted.tolist()}, rejected iterations "
          f"{rejected}; {moved_atoms} moving atoms moved, side-chain RMSD {res.sidechain_rmsd_moved.tolist()}; {bonds.shape[0]} bond lengths off by {worst:.2e}")
    assert worst < 1e-3 and int(res.accepted.max()) >= 1 and moved_atoms >= 1 and rejected >= 1
    assert torch.allclose(res.sidechain_rmsd_moved.double(), (res.atom_pos[:, mov].double() - apos[:, mov].double()).pow(2).sum(-1).mean(-1).sqrt(), atol=1e-6)
    sc_after = mz.scorer.score(res.lig_pos, res.atom_pos)
    assert torch.equal(sc_after.total, res.scores_after.total) and torch.allclose(sc_after.inter, res.energy_after[:, 0], rtol=1e-12)
    # the inputs are untouched; a NaN pose or a NaN moving atom is kept bit for bit and touches no other sample
    for where in ("x", "y"):
        bx, by = lig.clone(), apos.clone()
        if where == "x":
            bx[1, 3, 0] = float("nan")
        else:
            by[1, int(mov[0]), 2] = float("nan")
        got = mz.minimize(bx, by)
        assert int(got.accepted[1]) == 0 and torch.equal(bits32(got.lig_pos[1]), bits32(bx[1])) and torch.equal(bits32(got.atom_pos[1]), bits32(by[1]))
        assert bool(torch.isnan(got.energy_after[1, 5]))
        for s in (0, 2):
            assert torch.equal(bits32(got.lig_pos[s]), bits32(res.lig_pos[s])) and torch.equal(got.energy_after[s], res.energy_after[s])


def test_without_side_chain_bonds_it_is_pose_minimizer_bit_for_bit():
    g, lig, apos = small_flexible_case()
    g0 = make_3dpf_complex(seed=2, flexible_sidechains=True, n_lig=12, n_rec=8)
    g0["flexResidues"] = Store(edge_idx=torch.zeros(0, 2, dtype=torch.long), subcomponents=torch.zeros(0, dtype=torch.long),
                               subcomponentsMapping=torch.zeros(0, 2, dtype=torch.long))
    cfg = M.MinimizeConfig(iterations=8, restraint=0.2, sidechain_restraint=0.5)
    fx = MF.FlexPoseMinimizer(g0, config=cfg)
    assert fx.flexible and fx.sc.n_sc == 0 and fx.sc.n_mov == 0
    h1, h2 = [], []
    a, b = fx.minimize(lig, apos, history=h1), M.PoseMinimizer(g0, config=cfg).minimize(lig, apos, history=h2)
    assert torch.equal(bits32(a.lig_pos), bits32(b.lig_pos)) and torch.equal(a.accepted, b.accepted) and int(b.accepted.sum()) >= 1
    assert torch.equal(a.energy_after[:, [0, 1, 3, 5]], b.energy_after) and torch.equal(a.energy_before[:, [0, 1, 3, 5]], b.energy_before)
    assert torch.equal(torch.stack(h1), torch.stack(h2)) and torch.equal(bits32(a.atom_pos), bits32(apos))
    assert torch.equal(a.energy_after[:, [2, 4]], torch.zeros(3, 2, dtype=torch.float64))
    # a graph without flexResidues is handed to PoseMinimizer unchanged
    rigid = make_3dpf_complex(seed=2, flexible_sidechains=False, n_lig=12, n_rec=8)
    fr = MF.FlexPoseMinimizer(rigid, config=cfg)
    out = fr.minimize(lig, apos)
    assert not fr.flexible and isinstance(out, M.MinimizeResult) and torch.equal(bits32(out.lig_pos), bits32(b.lig_pos))


def test_the_restraint_holds_the_side_chains_back():
    g, lig, apos = small_flexible_case()
    free = MF.FlexPoseMinimizer(g, config=M.MinimizeConfig(iterations=10)).minimize(lig, apos)
    held = MF.FlexPoseMinimizer(g, config=M.MinimizeConfig(iterations=10, sidechain_restraint=50.0)).minimize(lig, apos)
    print("side-chain RMSD free", free.sidechain_rmsd_moved.tolist(), "held", held.sidechain_rmsd_moved.tolist())
    assert bool((held.sidechain_rmsd_moved <= free.sidechain_rmsd_moved).all()) and bool((held.energy_after[:, 4] >= 0).all())
    assert torch.equal(free.energy_after[:, 4], torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="sidechain_restraint"):
        MF.FlexPoseMinimizer(g, config=M.MinimizeConfig(sidechain_restraint=-1.0))


# ---------------------------------------------------------------------------------------------- 4. ABI
def test_entry_is_declared_exported_built_and_guarded():
    header = open(os.path.join(ROOT, "include", "ddp_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(ddp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert "ddp_pose_minimize_flex" in declared and "ddp_pose_minimize_flex" in L.EXPORTS and set(L.EXPORTS) == declared
    assert "#define DDP_ABI_VERSION 17" in header and "ddp_minimize_flex_args_t" in header
    for name in ("DDP_MINIMIZE_FLEX_MAX_MOVING", "DDP_MINIMIZE_FLEX_MAX_BONDS", "DDP_MINIMIZE_FLEX_MAX_STATE_BYTES"):
        assert f"#define {name} {getattr(L, name)}" in header, name
    build = __import__("diffdock_pocket_amd.build", fromlist=["SOURCES"])
    assert "ddp_minimize_flex.hip" in build.SOURCES and os.path.exists(os.path.join(os.path.dirname(build.__file__), "csrc", "ddp_minimize_flex.hip"))
    # the plan of the header: 18496 fixed bytes + the per-atom state stay inside 64 KiB, and the 3dpf fixture fits with room
    assert 18496 + L.DDP_MINIMIZE_FLEX_MAX_STATE_BYTES <= 64 * 1024 and L.flex_state_bytes(37, 37, 17) == 89 * 37 + 81 * 37 + 4 * 17
    assert L.flex_state_bytes(100, L.DDP_MINIMIZE_FLEX_MAX_MOVING, L.DDP_MINIMIZE_FLEX_MAX_BONDS) <= L.DDP_MINIMIZE_FLEX_MAX_STATE_BYTES
    assert os.path.exists(L.LIB_PATH), "build the library first (python -m diffdock_pocket_amd.build)"
    lib = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(lib, "ddp_pose_minimize_flex")
    lib.ddp_abi_version.restype = ctypes.c_int
    assert lib.ddp_abi_version() == 17
    # the ctypes mirror: ddp_minimize_args_t's fields first (the shared code reads them by name), then 1 pointer, 4 int32, 5 pointers,
    # 1 double, 1 pointer
    assert L.MinimizeFlexArgs._fields_[:len(L.MinimizeArgs._fields_)] == L.MinimizeArgs._fields_
    assert ctypes.sizeof(L.MinimizeFlexArgs) == ctypes.sizeof(L.MinimizeArgs) + 8 + 16 + 5 * 8 + 8 + 8
    body = header[header.index("typedef struct {", header.index("DDP_MINIMIZE_FLEX_MAX_STATE_BYTES 47040")):header.index("} ddp_minimize_flex_args_t;")]
    fields = re.findall(r"([a-z_0-9]+)(?=\s*[,;])", re.sub(r"/\*.*?\*/", "", body))
    assert fields == [f[0] for f in L.MinimizeFlexArgs._fields_], fields
    # the host-side checks of the entry need no device: they return before any launch
    fn = lib.ddp_pose_minimize_flex
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    A = L.MinimizeFlexArgs
    assert fn(None, None) == -1 and fn(ctypes.byref(A(n_samples=0)), None) == 0
    ok = dict(n_samples=1, n=4, m=8, rec_stride=24)
    assert fn(ctypes.byref(A(**dict(ok, n=L.DDP_MINIMIZE_MAX_ATOMS + 1))), None) == -2
    assert fn(ctypes.byref(A(**dict(ok, n_tor=L.DDP_MINIMIZE_MAX_TORSIONS + 1))), None) == -2
    assert fn(ctypes.byref(A(**dict(ok, n_mov=L.DDP_MINIMIZE_FLEX_MAX_MOVING + 1))), None) == -2
    assert fn(ctypes.byref(A(**dict(ok, n_sc=L.DDP_MINIMIZE_FLEX_MAX_BONDS + 1))), None) == -2
    assert L.flex_state_bytes(512, 19, 0) > L.DDP_MINIMIZE_FLEX_MAX_STATE_BYTES >= L.flex_state_bytes(512, 18, 0)
    assert fn(ctypes.byref(A(**dict(ok, n=512, n_mov=19))), None) == -2
    assert fn(ctypes.byref(A(**dict(ok, n=512, n_mov=18))), None) == -1            # inside the limits: on to the null pointers
    assert fn(ctypes.byref(A(**ok)), None) == -1                                    # null pointers
    for bad in (dict(rec_stride=0), dict(rec_stride=23), dict(n_samples=-1), dict(n_mov=-1), dict(n_sc=-1), dict(n_sub=-1)):
        assert fn(ctypes.byref(A(**dict(ok, **bad))), None) == -1, bad
    lib.ddp_last_error.restype = ctypes.c_char_p
    assert fn(ctypes.byref(A(**dict(ok, rec_stride=0))), None) == -1 and b"rec_stride" in lib.ddp_last_error()


# ---------------------------------------------------------------------------------------------- 5. flags and driver
def test_flags_parse_and_default_to_off(tmp_path, capsys):
    p = INF._parser()
    a = p.parse_args([])
    assert a.minimize_sidechains is False and a.minimize_sidechain_restraint == 0.0 and a.minimize_poses is False
    a = p.parse_args(["--minimize_sidechains", "--minimize_sidechain_restraint", "0.5"])
    assert a.minimize_sidechains is True and a.minimize_sidechain_restraint == 0.5
    c = M.MinimizeConfig()
    assert c.sidechains is False and c.sidechain_restraint == 0.0
    (tmp_path / "model_parameters.yml").write_text("{}\n")
    with pytest.raises(SystemExit) as e:
        INF.main(["--protein_path", "p.pdb", "--ligand", "l.sdf", "--model_dir", str(tmp_path), "--minimize_sidechain_restraint", "-1"])
    assert e.value.code == 2 and "--minimize_sidechain_restraint must not be negative" in capsys.readouterr().err


def test_run_csv_minimises_side_chains_of_flexible_rows_only(tmp_path):
    p = tmp_path / "complexes.csv"
    p.write_text(CSV)
    plain = _run(str(p), str(tmp_path / "plain"), minimize_poses=M.MinimizeConfig(iterations=3))
    joint = _run(str(p), str(tmp_path / "joint"), minimize_poses=M.MinimizeConfig(iterations=3, sidechains=True, sidechain_restraint=0.1))
    new_files = {"minimized_sidechains.csv"} | {f"rank{k}_minimized_protein.pdb" for k in range(1, 5)}
    for row, (a, b) in enumerate(zip(plain, joint)):
        assert a.skipped is None and b.skipped is None, (a.skipped, b.skipped)
        assert isinstance(a.minimized, M.MinimizeResult) and torch.equal(a.ligand_pos, b.ligand_pos) and torch.equal(a.order, b.order)
        old = {os.path.basename(f): f for f in a.files}
        new = {os.path.basename(f): f for f in b.files}
        assert set(os.listdir(os.path.dirname(b.files[0]))) == set(new)
        if row == 1:            # the rigid row: nothing new, every file as without the flag
            assert isinstance(b.minimized, M.MinimizeResult) and set(new) == set(old)
            for name, path in old.items():
                assert open(path, "rb").read() == open(new[name], "rb").read(), name
            assert torch.equal(bits32(a.minimized_pos), bits32(b.minimized_pos))
            continue
        mr = b.minimized
        assert isinstance(mr, MF.FlexMinimizeResult) and set(new) - set(old) == new_files and set(old) <= set(new)
        for name, path in old.items():
            if "minimized" not in name:
                assert open(path, "rb").read() == open(new[name], "rb").read(), name
        assert torch.equal(mr.lig_pos, b.minimized_pos) and mr.atom_pos.shape[0] == 4 and mr.energy_after.shape == (4, 6)
        assert bool((mr.energy_after[:, 5] <= mr.energy_before[:, 5]).all())
        rows = _rows(new["minimized.csv"])
        assert list(rows[0].keys()) == O.MINIMIZED_COLUMNS and len(rows) == 4
        sc_rows = _rows(new["minimized_sidechains.csv"])
        assert list(sc_rows[0].keys()) == ["rank", "sample", "sc_before", "sc_after", "sidechain_restraint_after", "sidechain_rmsd_moved"]
        for r in range(4):
            assert int(rows[r]["sample"]) == int(sc_rows[r]["sample"]) == int(b.order[r]) and int(sc_rows[r]["rank"]) == r + 1
            for got, val in ((rows[r]["energy_after"], mr.energy_after[r, 5]), (rows[r]["energy_before"], mr.energy_before[r, 5]),
                             (rows[r]["restraint_after"], mr.energy_after[r, 3]), (rows[r]["total_after"], mr.scores_after.total[r]),
                             (sc_rows[r]["sc_before"], mr.energy_before[r, 2]), (sc_rows[r]["sc_after"], mr.energy_after[r, 2]),
                             (sc_rows[r]["sidechain_restraint_after"], mr.energy_after[r, 4])):
                assert abs(float(got) - float(val)) <= 1e-5 * abs(float(val)) + 1e-12
            assert abs(float(sc_rows[r]["sidechain_rmsd_moved"]) - float(mr.sidechain_rmsd_moved[r])) < 1e-4
        # the written receptor carries the minimised side chains: it differs from the sampled one exactly where an atom moved
        moved = [r for r in range(4) if float(mr.sidechain_rmsd_moved[r]) > 1e-3]
        assert moved, "no side chain moved in the miniature"
        sampled = [n for n in old if n.endswith("_protein.pdb") and n.startswith(f"rank{moved[0] + 1}_")]
        assert open(old[sampled[0]]).read() != open(new[f"rank{moved[0] + 1}_minimized_protein.pdb"]).read()
        # rank_by minimized_score orders by the total of the minimised pose against its minimised side chains
    ranked = _run(str(p), str(tmp_path / "ranked"), rank_by="minimized_score",
                  minimize_poses=M.MinimizeConfig(iterations=3, sidechains=True, sidechain_restraint=0.1))[0]
    t = ranked.minimized.scores_after.total
    assert bool((t[:-1] <= t[1:]).all()) and isinstance(ranked.minimized, MF.FlexMinimizeResult)
    inv_a, inv_b = torch.argsort(joint[0].order), torch.argsort(ranked.order)
    assert torch.equal(bits32(joint[0].minimized.atom_pos[inv_a]), bits32(ranked.minimized.atom_pos[inv_b]))
