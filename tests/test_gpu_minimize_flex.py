"""csrc/ddp_minimize_flex.hip on the device: ddp_pose_minimize_flex with iterations = 0 against the NumPy fp64 restatement of
tests/flexmin_ref.py within the derived bound (the edges of the 1024-atom receptor tile, moving atoms on either side of them, an untyped
moving atom, per-sample receptors); bit equality with ddp_pose_minimize without side chains and with ddp_pose_score at iterations = 0;
one iteration against the CPU form with accepts and rejects; resumability, determinism and batch independence, bit for bit; NaN
containment and what is written to rec; the limits, the return codes and the fall-back above them; run_csv on the device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import flexmin_ref as F
from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import launch as LA
from diffdock_pocket_amd import minimize as M
from diffdock_pocket_amd import minimize_flex as MF
from diffdock_pocket_amd import refine as R
from diffdock_pocket_amd.sampler import apply_sidechain_torsions, modify_conformer
from test_evaluation_cpu import graph_3dpf
from test_minimize_cpu import bits32, chain_case
from test_scoring_cpu import CFG, perturbed_poses

pytestmark = pytest.mark.gpu
TILE = 1024          # DDP_FX_TILE of csrc/ddp_minimize_flex.hip
_CACHE = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int64)


class Tables:
    """The side-chain tables of a flexmin_ref.random_case under the names launch.flex_tables reads."""

    def __init__(self, c, n_mov=None, n_sc=None):
        n_mov = len(c["mov"]) if n_mov is None else n_mov
        n_sc = len(c["edge"]) if n_sc is None else n_sc
        self.mov, self.pairs = torch.from_numpy(c["mov"][:n_mov]), torch.from_numpy(c["sc_pairs"][:n_mov])
        self.edge_idx, self.mapping = torch.from_numpy(c["edge"][:n_sc]), torch.from_numpy(c["mapping"][:n_sc])
        self.sub = torch.from_numpy(c["sub"])


def device_case(c, dev):
    t = {k: torch.from_numpy(c[k]).to(dev) for k in ("x", "y", "x0", "y0", "lig_r", "lig_f", "rec_r", "rec_f")}
    t["pairs"] = None if c["pairs"] is None else torch.from_numpy(c["pairs"]).to(dev)
    t["tables"] = LA.flex_tables(Tables(c), c["y"].shape[1], dev)
    return t


def _raw(t, iterations, k=0.0, k_sc=0.0, bonds=None, mask=None, x=None, y=None, step=None, acc=None, history=False, tables=None):
    """ddp_pose_minimize_flex on CLONES of the device state (x, y, step, accepted); returns a dict of everything it writes."""
    x = (t["x"] if x is None else x).clone()
    y = (t["y"] if y is None else y).clone()
    S, n, dev = x.shape[0], x.shape[1], x.device
    tables = t["tables"] if tables is None else tables
    step = torch.ones(S, dtype=torch.float64, device=dev) if step is None else step.clone()
    acc = torch.zeros(S, dtype=torch.int32, device=dev) if acc is None else acc.clone()
    e0 = torch.full((S, 6), -7.0, dtype=torch.float64, device=dev)
    e1 = torch.full((S, 6), -7.0, dtype=torch.float64, device=dev)
    h = torch.full((iterations + 1, S), -7.0, dtype=torch.float64, device=dev) if history else None
    gx = torch.full((S, n, 3), -7.0, dtype=torch.float64, device=dev)
    gy = torch.full((S, tables["mov"].shape[0], 3), -7.0, dtype=torch.float64, device=dev)
    LA.pose_minimize_flex(x, t["x0"], t["lig_r"], t["lig_f"], y, t["y0"], t["rec_r"], t["rec_f"], CFG, t["pairs"], bonds, mask, tables, step,
                          acc, e0, e1, iterations, restraint=k, restraint_sc=k_sc, history=h, grad=gx, grad_mov=gy)
    return dict(x=x, y=y, step=step, acc=acc, e0=e0, e1=e1, h=h, gx=gx, gy=gy)


def same_state(a, b, what):
    assert torch.equal(bits32(a["x"]), bits32(b["x"])) and torch.equal(bits32(a["y"]), bits32(b["y"])), what + ": pos / rec"
    assert torch.equal(_bits(a["step"]), _bits(b["step"])) and torch.equal(a["acc"], b["acc"]), what + ": step / accepted"
    assert torch.equal(_bits(a["e1"]), _bits(b["e1"])), what + ": energy_out"
    assert torch.equal(_bits(a["gx"]), _bits(b["gx"])) and torch.equal(_bits(a["gy"]), _bits(b["gy"])), what + ": gradients at exit"


def flex_fixture():
    """(graph, 16 poses, atom_pos [16, m, 3]) on the real 3dpf complex with the flexible residues A:160, A:193 and A:197 (every atom
    typed; 7 moving atoms, 4 side-chain bonds): the 16 perturbed ligand poses of the scoring fixture, the side chains of every pose
    perturbed by chi noise N(0, 0.3 rad) of torch.Generator().manual_seed(4); built once."""
    if "fix" not in _CACHE:
        g, _ = graph_3dpf("A:160-A:193-A:197")
        fr = g["flexResidues"]
        chi = 0.3 * torch.randn(16, fr.edge_idx.shape[0], generator=torch.Generator().manual_seed(4))
        apos = apply_sidechain_torsions(g["atom"].pos.float()[None].repeat(16, 1, 1), fr.edge_idx, fr.subcomponents, fr.subcomponentsMapping, chi)
        _CACHE["fix"] = (g, perturbed_poses(), apos.contiguous())
    return _CACHE["fix"]


# ---------------------------------------------------------------------------------------------- 1. iterations = 0 against the restatement
CASES = [  # S, n, m, n_mov, n_sc, options of flexmin_ref.random_case
    (1, 1, 1, 1, 0, {}),
    (3, 37, 1, 1, 0, {}),
    (1, 1, TILE - 1, 5, 0, dict(moving_at=[TILE - 2])),
    (3, 5, TILE - 1, 4, 1, dict(moving_at=[0, TILE - 2])),
    (3, 37, TILE + 1, 5, 17, dict(moving_at=[TILE - 1, TILE])),
    (1, 37, TILE + 1, 37, 17, dict(moving_at=[TILE - 1, TILE], untyped_moving=True)),
    (3, 5, TILE + 1, 37, 1, dict(with_pairs=False)),
    (1, 5, TILE + 1, 1, 1, dict(moving_at=[TILE])),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "S{}-n{}-m{}-mov{}-sc{}".format(*c[:5]))
def test_zero_iterations_match_the_fp64_restatement(case):
    """energy_in [S, 6], grad and grad_mov against flexmin_ref.energy within flexmin_ref.bounds, 256 eps (P + 1) max(1, largest
    |summand|) per entry.  Every case has per-sample receptors that differ; random_case redraws until no pair, cross, self or sc, lies
    within 1e-6 A of the cutoff.  Nothing but the outputs is written."""
    dev = _dev()
    S, n, m, n_mov, n_sc, opt = case
    c = F.random_case(S, n, m, n_mov, n_sc, seed=17 * n + m + 3 * n_mov + n_sc, **opt)
    assert S == 1 or not np.array_equal(c["y"][0], c["y"][1])
    t = device_case(c, dev)
    out = _raw(t, 0, c["k"], c["k_sc"], history=True)
    torch.cuda.synchronize()
    ref = c["ref"]
    be, bgx, bgy = F.bounds(ref)
    err = np.abs(out["e0"].cpu().numpy() - ref["energy"])
    ex, ey = np.abs(out["gx"].cpu().numpy() - ref["grad_x"]), np.abs(out["gy"].cpu().numpy() - ref["grad_y"])
    print(f"worst |err| / bound: energy {float((err / be).max()):.3e}, dE/dx {float((ex / bgx[:, None, None]).max()):.3e}, "
          f"dE/dy {float((ey / bgy[:, None, None]).max()):.3e}; pairs inter / intra / sc {ref['n_pairs'][0, :3].tolist()}")
    assert (err <= be).all(), err / be
    assert (ex <= bgx[:, None, None]).all() and (ey <= bgy[:, None, None]).all()
    assert torch.equal(bits32(out["x"]), bits32(t["x"])) and torch.equal(bits32(out["y"]), bits32(t["y"]))
    assert torch.equal(out["step"], torch.ones_like(out["step"])) and int(out["acc"].sum()) == 0
    assert torch.equal(_bits(out["e0"]), _bits(out["e1"])) and torch.equal(_bits(out["h"][0]), _bits(out["e0"][:, 5]))
    if opt.get("untyped_moving"):       # the untyped moving atom feels the restraint only
        dy = c["y"][:, c["mov"][0]].astype(np.float64) - c["y0"][:, c["mov"][0]].astype(np.float64)
        assert np.allclose(out["gy"][:, 0].cpu().numpy(), 2 * c["k_sc"] / n_mov * dy, rtol=1e-13, atol=0)


# ---------------------------------------------------------------------------------------------- 2. the existing entries' bits
@pytest.mark.parametrize("T", [0, 5])
def test_without_side_chains_ten_iterations_equal_ddp_pose_minimize_bit_for_bit(T):
    dev = _dev()
    x, lig_r, lig_f, rec, rec_r, rec_f, pairs, bonds, mask = (a.to(dev) for a in chain_case(3, 37, T, TILE + 1, 90 + T))
    rec = rec[None].repeat(3, 1, 1).contiguous()
    rec[1] += 0.05
    S = 3
    step, acc = torch.ones(S, dtype=torch.float64, device=dev), torch.zeros(S, dtype=torch.int32, device=dev)
    e0, e1 = torch.empty(S, 4, dtype=torch.float64, device=dev), torch.empty(S, 4, dtype=torch.float64, device=dev)
    h = torch.empty(11, S, dtype=torch.float64, device=dev)
    pos = x.clone()
    LA.pose_minimize(pos, x, lig_r, lig_f, rec, rec_r, rec_f, CFG, pairs, bonds if T else None, mask if T else None, step, acc, e0, e1, 10,
                     restraint=0.1, history=h)
    empty = LA.flex_tables(Tables(dict(mov=np.zeros(0, np.int64), sc_pairs=np.zeros((0, TILE + 1), np.uint8), edge=np.zeros((0, 2), np.int64),
                                       mapping=np.zeros((0, 2), np.int64), sub=np.zeros(0, np.int64))), TILE + 1, dev)
    t = dict(x=x, y=rec, x0=x, y0=rec, lig_r=lig_r, lig_f=lig_f, rec_r=rec_r, rec_f=rec_f, pairs=pairs, tables=empty)
    out = _raw(t, 10, 0.1, 0.4, bonds if T else None, mask if T else None, history=True)
    torch.cuda.synchronize()
    assert torch.equal(bits32(out["x"]), bits32(pos)) and torch.equal(_bits(out["step"]), _bits(step)) and torch.equal(out["acc"], acc)
    assert torch.equal(_bits(out["e1"][:, [0, 1, 3, 5]]), _bits(e1)) and torch.equal(_bits(out["e0"][:, [0, 1, 3, 5]]), _bits(e0))
    assert torch.equal(_bits(out["h"]), _bits(h)) and int(acc.sum()) >= 1 and torch.equal(bits32(out["y"]), bits32(rec))
    assert torch.equal(out["e1"][:, [2, 4]], torch.zeros(S, 2, dtype=torch.float64, device=dev))


def test_zero_iterations_with_moving_atoms_equal_ddp_pose_score_bit_for_bit():
    """The moving atoms go into the receptor tile from LDS with the coordinates global memory has: inter, intra and the ligand gradient
    are the bits of ddp_pose_score on the same coordinates."""
    dev = _dev()
    c = F.random_case(3, 37, TILE + 1, 37, 17, seed=8, moving_at=[TILE - 1, TILE])
    t = device_case(c, dev)
    out = _raw(t, 0, 0.0, 0.3)
    e7, gs = LA.pose_score(t["x"], t["lig_r"], t["lig_f"], t["y"], t["rec_r"], t["rec_f"], CFG, 1.0, t["pairs"], with_grad=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out["e0"][:, 0:2]), _bits(e7[:, 4:6])) and torch.equal(_bits(out["gx"]), _bits(gs))
    assert bool(torch.isfinite(gs).all()) and float(out["e0"][:, 2].abs().min()) > 0


# ---------------------------------------------------------------------------------------------- 3. one iteration against the CPU form
def test_one_iteration_matches_the_cpu_form():
    """Per-sample input steps 2^-3 ... 2^9 on the 16 poses of flex_fixture: accepts and rejects both occur, and every decision is
    clear of rounding on the CPU side (|dE| > 1e-6 |E|).  Energies at rtol 1e-9: energy_in, energy_out of a rejected pose, and
    energy_out of an accepted pose against the CPU form's energy of the RETURNED state (the device's own trial differs from the CPU
    trial in the last bits of its fp32 coordinates); accepted coordinates of x and y within 2e-5 max|coordinate| of the CPU trial.
    A sample that accepted nothing has its pose and its receptor untouched, bit for bit; static atoms are untouched everywhere."""
    dev = _dev()
    g, x, y = flex_fixture()
    cpu, gpu = MF.FlexPoseMinimizer(g), MF.FlexPoseMinimizer(g, dev)
    step = torch.pow(2.0, torch.linspace(-3, 9, 16, dtype=torch.float64))
    zero = torch.zeros(16, dtype=torch.int32)
    xc, yc, sc, ac, e0c, e1c = cpu.advance(x, y, x, y, step, zero, 1)
    # the CPU trial and its energy, restated
    e, gx, gy = cpu.energy(x, y)
    d_tr, d_rot, d_tor = R.direction_torch(x, gx, cpu.rigid.bonds, cpu.rigid.mask_rotate)
    d_sc = MF.direction_sc_torch(y, gy, cpu.sc.mov, cpu.sc.edge_idx, cpu.sc.sub, cpu.sc.mapping)
    xt = modify_conformer(x, (step[:, None] * d_tr).float(), (step[:, None] * d_rot).float(), (step[:, None] * d_tor).float(),
                          cpu.rigid.bonds, cpu.rigid.rot_idx)
    yt = apply_sidechain_torsions(y, cpu.sc.edge_idx, cpu.sc.sub, cpu.sc.mapping, (step[:, None] * d_sc).float())
    et, _, _ = cpu.energy(xt, yt, anchor=x, atom_anchor=y)
    assert bool(((et[:, 5] - e[:, 5]).abs() > 1e-6 * e[:, 5].abs()).all()), "a decision of the fixture is not clear of rounding"
    take = et[:, 5] < e[:, 5]
    assert torch.equal(take.to(torch.int32), ac) and 0 < int(take.sum()) < 16, take
    assert float(d_sc.abs().max()) > 0 and not torch.equal(bits32(yt[take]), bits32(y[take])), "the side chains do not move in the fixture"
    xd, yd, sd, ad, e0d, e1d = (v.cpu() for v in gpu.advance(x.to(dev), y.to(dev), x.to(dev), y.to(dev), step.to(dev), zero.to(dev), 1))
    assert torch.equal(ad, ac) and torch.equal(sd, sc)
    assert torch.equal(bits32(xd[~take]), bits32(x[~take])) and torch.equal(bits32(yd[~take]), bits32(y[~take])), "a rejected state changed"
    wx, wy = float((xd[take].double() - xt[take].double()).abs().max()), float((yd[take].double() - yt[take].double()).abs().max())
    sx, sy = float(xt.abs().max()), float(yt.abs().max())
    print(f"accepted {int(take.sum())} of 16; accepted x off the CPU trial by {wx:.2e} (bound {2e-5 * sx:.2e}), y by {wy:.2e} (bound {2e-5 * sy:.2e})")
    assert wx <= 2e-5 * sx and wy <= 2e-5 * sy
    mov = cpu.sc.mov
    static = torch.ones(y.shape[1], dtype=torch.bool)
    static[mov] = False
    assert torch.equal(bits32(yd[:, static]), bits32(y[:, static])) and not torch.equal(bits32(yd[take][:, mov]), bits32(y[take][:, mov]))

    def close(a, b):
        return bool(((a - b).abs() <= 1e-9 * b.abs() + 1e-12).all())

    assert close(e0d, e0c) and close(e1d[~take], e1c[~take])
    e_ret, _, _ = cpu.energy(xd, yd, anchor=x, atom_anchor=y)
    assert close(e1d, e_ret), float(((e1d - e_ret).abs() / e_ret.abs().clamp(min=1e-3)).max())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 4. resumable, deterministic, independent
@pytest.mark.parametrize("n_sc", [0, 1, 5])
def test_split_calls_repeated_launches_and_batch_rows_give_the_same_bits(n_sc):
    """Two launches; 5 + 7 iterations against 12 on the state left in memory; row s of the batch against the one-pose launch.  The
    ligand is a chain with 2 rotatable bonds; 6 moving atoms, one of them in the second receptor tile."""
    dev = _dev()
    m = TILE + 1
    c = F.random_case(3, 12, m, 6, 5, seed=60, moving_at=[TILE])
    _, _, _, _, _, _, _, bonds, mask = chain_case(3, 12, 2, 4, 1)
    c["y"] *= 0.6       # a crowded receptor: the side chains feel their neighbours
    c["y0"] = c["y"].copy()
    t = device_case(c, dev)
    t["x0"] = t["x"]
    tables = LA.flex_tables(Tables(c, n_sc=n_sc), m, dev)
    kw = dict(k=0.1, k_sc=0.05, bonds=bonds.to(dev), mask=mask.to(dev), tables=tables)
    whole, again = _raw(t, 12, history=True, **kw), _raw(t, 12, history=True, **kw)
    same_state(whole, again, "two launches")
    assert torch.equal(_bits(whole["h"]), _bits(again["h"]))
    a = _raw(t, 5, **kw)
    b = _raw(t, 7, x=a["x"], y=a["y"], step=a["step"], acc=a["acc"], **kw)
    same_state(whole, b, "5 + 7")
    assert torch.equal(_bits(b["e0"]), _bits(a["e1"])) and torch.equal(_bits(whole["e0"]), _bits(a["e0"]))
    for s in range(3):
        ts = {k: (v[s:s + 1] if k in ("x", "y", "x0", "y0") else v) for k, v in t.items()}
        one = _raw(ts, 12, **kw)
        for k in ("x", "y", "e1", "gx", "gy", "step"):
            assert torch.equal(whole[k][s:s + 1].contiguous().view(torch.uint8), one[k].contiguous().view(torch.uint8)), (s, k)
        assert int(one["acc"][0]) == int(whole["acc"][s])
    h = whole["h"]
    static = torch.ones(m, dtype=torch.bool, device=dev)
    static[tables["mov"].long()] = False
    moved = bool((bits32(whole["y"]) != bits32(t["y"])).any())
    print(f"n_sc={n_sc}: accepted {whole['acc'].tolist()}, E {h[0].tolist()} -> {h[-1].tolist()}, side chains moved: {moved}")
    assert bool((h[1:] <= h[:-1]).all()) and int(whole["acc"].sum()) >= 1
    assert torch.equal(bits32(whole["y"][:, static]), bits32(t["y"][:, static])) and (n_sc > 0 or not moved)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 5. NaN, what is written
def test_a_nan_is_kept_bit_for_bit_and_rec_is_written_only_after_an_accept():
    dev = _dev()
    g, x, y = flex_fixture()
    x, y = x[:4].to(dev), y[:4].to(dev)
    mz = MF.FlexPoseMinimizer(g, dev, config=M.MinimizeConfig(iterations=6))
    clean = mz.minimize(x, y)
    mov = mz.sc.mov.to(dev)
    static = torch.ones(y.shape[1], dtype=torch.bool, device=dev)
    static[mov] = False
    assert torch.equal(bits32(clean.atom_pos[:, static]), bits32(y[:, static])) and bool((clean.accepted >= 1).all())
    assert bool((bits32(clean.atom_pos[:, mov]) != bits32(y[:, mov])).any())
    for where in ("ligand", "moving atom"):
        bx, by = x.clone(), y.clone()
        if where == "ligand":
            bx[2, 5, 1] = float("nan")
        else:
            by[2, int(mov[3]), 0] = float("nan")
        got = mz.minimize(bx, by)
        torch.cuda.synchronize()
        assert int(got.accepted[2]) == 0 and torch.equal(bits32(got.lig_pos[2]), bits32(bx[2])) and torch.equal(bits32(got.atom_pos[2]), bits32(by[2])), where
        assert bool(torch.isnan(got.energy_before[2, 5])) and bool(torch.isnan(got.energy_after[2, 5]))
        for s in (0, 1, 3):
            assert torch.equal(bits32(got.lig_pos[s]), bits32(clean.lig_pos[s])) and torch.equal(bits32(got.atom_pos[s]), bits32(clean.atom_pos[s])), where
            assert torch.equal(_bits(got.energy_after[s]), _bits(clean.energy_after[s])) and int(got.accepted[s]) == int(clean.accepted[s])


# ---------------------------------------------------------------------------------------------- 6. limits
def test_limits_return_codes_and_the_fall_back():
    dev = _dev()
    lib = L.load()
    c = F.random_case(2, 8, 20, 4, 2, seed=3)
    t = device_case(c, dev)
    tb = t["tables"]
    pos, rec = t["x"].clone(), t["y"].clone()
    step, acc = torch.ones(2, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    e0 = torch.full((2, 6), -7.0, dtype=torch.float64, device=dev)
    e1 = torch.full((2, 6), -7.0, dtype=torch.float64, device=dev)

    def rc(**kw):
        a = L.MinimizeFlexArgs(n_samples=2, n=8, m=20, rec_stride=60, n_tor=0, iterations=2, pos=pos.data_ptr(), anchor=t["x0"].data_ptr(),
                               lig_radii=t["lig_r"].data_ptr(), lig_flags=t["lig_f"].data_ptr(), rec=rec.data_ptr(), rec_radii=t["rec_r"].data_ptr(),
                               rec_flags=t["rec_f"].data_ptr(), self_pairs=t["pairs"].data_ptr(), cutoff=8.0, gauss_offset=0.0, gauss_width=0.8,
                               hydrophobic_good=0.0, hydrophobic_bad=2.5, hbond_good=-0.6, hbond_bad=0.0, w_gauss=-0.045, w_repulsion=0.8,
                               w_hydrophobic=-0.035, w_hbond=-0.6, restraint=0.0, grow=2.0, shrink=0.5, step_max=1024.0, step=step.data_ptr(),
                               accepted=acc.data_ptr(), energy_in=e0.data_ptr(), energy_out=e1.data_ptr(), rec_anchor=t["y0"].data_ptr(),
                               n_mov=4, n_sc=2, n_sub=int(tb["sub"].shape[0]), mov=tb["mov"].data_ptr(), sc_edge_idx=tb["edge_idx"].data_ptr(),
                               sc_sub=tb["sub"].data_ptr(), sc_map=tb["mapping"].data_ptr(), sc_pairs=tb["pairs"].data_ptr(), restraint_sc=0.0)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.ddp_pose_minimize_flex(ctypes.byref(a), LA.stream())

    # DDP_ELIMIT just above each limit, without a launch
    assert rc(n_mov=L.DDP_MINIMIZE_FLEX_MAX_MOVING + 1) == -2 and rc(n_sc=L.DDP_MINIMIZE_FLEX_MAX_BONDS + 1) == -2
    assert rc(n=L.DDP_MINIMIZE_MAX_ATOMS + 1) == -2 and rc(n_tor=L.DDP_MINIMIZE_MAX_TORSIONS + 1) == -2
    assert L.flex_state_bytes(512, 19, 0) == L.DDP_MINIMIZE_FLEX_MAX_STATE_BYTES + 67 and rc(n=512, n_mov=19) == -2
    for bad in (dict(rec_stride=0), dict(rec_stride=59), dict(pos=None), dict(anchor=None), dict(lig_radii=None), dict(lig_flags=None),
                dict(step=None), dict(accepted=None), dict(energy_in=None), dict(energy_out=None), dict(rec=None), dict(rec_radii=None),
                dict(rec_flags=None), dict(rec_anchor=None), dict(mov=None), dict(sc_pairs=None), dict(sc_edge_idx=None), dict(sc_map=None),
                dict(sc_sub=None), dict(n_tor=1), dict(n_mov=-1), dict(n_sc=-1), dict(n_sub=-1), dict(iterations=-1), dict(restraint_sc=-0.1),
                dict(restraint_sc=float("nan")), dict(restraint=-1.0), dict(cutoff=0.0), dict(n_samples=-1), dict(n=0)):
        assert rc(**bad) == -1, bad                                                                                   # DDP_EINVAL
    assert rc(n_samples=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(e0, torch.full_like(e0, -7.0)) and torch.equal(bits32(pos), bits32(t["x"])) and torch.equal(bits32(rec), bits32(t["y"])), "a guard launched"
    assert rc() == 0
    torch.cuda.synchronize()
    assert bool((e0 != -7.0).all()) and bool((e1 != -7.0).all())
    # tables that the device would have to skip never reach it
    bad_tables = Tables(c)
    bad_tables.sub = bad_tables.sub.clone()
    bad_tables.sub[0] = 20
    with pytest.raises(L.DdpError, match="outside"):
        LA.flex_tables(bad_tables, 20, dev)
    # more side-chain bonds than the kernel holds: the class warns once, naming the limit, and runs the CPU form on host copies
    g, x, y = _fixture_small()
    fr = g["flexResidues"]
    reps = L.DDP_MINIMIZE_FLEX_MAX_BONDS // int(fr.edge_idx.shape[0]) + 1
    sub, mp = fr.subcomponents, fr.subcomponentsMapping
    g["flexResidues"].edge_idx = fr.edge_idx.repeat(reps, 1)
    g["flexResidues"].subcomponentsMapping = torch.cat([mp + k * sub.shape[0] for k in range(reps)])
    g["flexResidues"].subcomponents = sub.repeat(reps)
    cfg = M.MinimizeConfig(iterations=2)
    big = MF.FlexPoseMinimizer(g, dev, config=cfg)
    assert big.sc.n_sc > L.DDP_MINIMIZE_FLEX_MAX_BONDS and not big.fused_available()
    M._warned.clear()
    with pytest.warns(UserWarning, match="DDP_MINIMIZE_FLEX_MAX_BONDS"):
        fell = big.minimize(x.to(dev), y.to(dev))
    want = MF.FlexPoseMinimizer(g, config=cfg).minimize(x, y)
    assert fell.lig_pos.is_cuda and torch.equal(bits32(fell.lig_pos.cpu()), bits32(want.lig_pos)) and torch.equal(bits32(fell.atom_pos.cpu()), bits32(want.atom_pos))
    assert torch.equal(fell.energy_after.cpu(), want.energy_after) and torch.equal(fell.accepted.cpu(), want.accepted)


def _fixture_small():
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    g = make_3dpf_complex(seed=2, flexible_sidechains=True, n_lig=12, n_rec=8)
    gen = torch.Generator().manual_seed(11)
    lig = (g["ligand"].pos.float()[None] + 0.3 * torch.randn(2, 12, 3, generator=gen)).contiguous()
    return g, lig, g["atom"].pos.float()[None].repeat(2, 1, 1).contiguous()


# ---------------------------------------------------------------------------------------------- 7. the driver on the device
def test_run_csv_minimises_side_chains_on_the_device(tmp_path):
    from test_gpu_trajectory import GOLDEN, _model_dir
    from diffdock_pocket_amd.sampler import SamplerConfig
    dev = _dev()
    model_dir = _model_dir(tmp_path, True)
    model, margs, sigma = INF._load_model(model_dir, "best_ema_inference_epoch_model.pt", dev)
    pdb, sdf = os.path.join(GOLDEN, "3dpf_protein.pdb"), os.path.join(GOLDEN, "3dpf_ligand.sdf")
    csv_path = tmp_path / "two.csv"
    csv_path.write_text("complex_name,experimental_protein,ligand,pocket_center_x,pocket_center_y,pocket_center_z,flexible_sidechains\n"
                        f"flex_a,{pdb},{sdf},,,,A:160-A:193-A:197\nflex_b,{pdb},{sdf},,,,A:160\n")
    gk = {k: getattr(margs, k) for k in ("receptor_radius", "c_alpha_max_neighbors", "remove_hs", "pocket_reduction", "pocket_buffer",
                                         "pocket_cutoff")}
    gk["flexdist"] = float(margs.flexdist)
    cfg = SamplerConfig(inference_steps=4, sigma=sigma, flexible_sidechains=True)
    out = INF.run_csv(str(csv_path), model, dev, samples_per_complex=3, inference_steps=4, seed=7, sampler_cfg=cfg, graph_kwargs=gk,
                      allow_zero_esm=True, out_dir=str(tmp_path / "out"), minimize_poses=M.MinimizeConfig(iterations=3, sidechains=True))
    assert len(out) == 2
    for res in out:
        assert res.skipped is None, res.skipped
        mr = res.minimized
        assert isinstance(mr, MF.FlexMinimizeResult) and not mr.lig_pos.is_cuda and mr.lig_pos.shape == res.ligand_pos.shape
        assert torch.equal(mr.lig_pos, res.minimized_pos) and bool((mr.energy_after[:, 5] <= mr.energy_before[:, 5]).all())
        names = {os.path.basename(f) for f in res.files}
        assert {"minimized.csv", "minimized_sidechains.csv"} | {f"rank{k}_minimized.sdf" for k in (1, 2, 3)} | \
               {f"rank{k}_minimized_protein.pdb" for k in (1, 2, 3)} <= names
        assert names == set(os.listdir(os.path.dirname(res.files[0])))
    torch.cuda.synchronize()
