"""diffdock_pocket_amd/minimize.py without a device: the energy and its gradient against scoring.score_torch, the NumPy restatement and
autograd; the invariants of a 50-iteration run on the 16 perturbed poses of the 3dpf fixture (computed once); the restraint; NaN
containment; iterations = 0; per-sample receptors on the flexible synthetic graph; the C entry's declaration, export, struct size
and launch-free guards; the flags and run_csv."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import vinardo_ref as V
from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import minimize as M
from diffdock_pocket_amd import outputs as O
from diffdock_pocket_amd import refine as R
from diffdock_pocket_amd import scoring as SC
from diffdock_pocket_amd.batch import HeteroBatch
from diffdock_pocket_amd.synthetic import make_3dpf_complex
from test_refine_cpu import rigid_fragments
from test_scoring_cpu import CFG, CSV, ROOT, _rows, _run, as_torch, fixture_3dpf, perturbed_poses

_CACHE = {}


# ---------------------------------------------------------------------------------------------- shared helpers and fixtures
def bits32(t):
    return t.contiguous().view(torch.int32)


def plain_rmsd(x, ref):
    return (x.double() - ref.double()).pow(2).sum(-1).mean(-1).sqrt()


def run_50():
    """(MinimizeResult, history [51, 16]) of the CPU form on the 16-pose fixture, full typed receptor, 50 iterations, k = 0; once."""
    if "run" not in _CACHE:
        g, _, full = fixture_3dpf()
        h = []
        res = M.PoseMinimizer(g, receptor=full, config=M.MinimizeConfig(iterations=50)).minimize(perturbed_poses(), history=h)
        _CACHE["run"] = (res, torch.stack(h))
    return _CACHE["run"]


def check_invariants(res, hist, x0, what):
    """The invariants the issue sets for a 50-iteration run on the fixture (host tensors); prints the measured values."""
    g, _, _ = fixture_3dpf()
    assert hist.shape == (51, 16) and bool((hist[1:] <= hist[:-1]).all()), "the history rises somewhere"
    assert torch.equal(hist[0], res.energy_before[:, 3]) and torch.equal(hist[-1], res.energy_after[:, 3])
    assert bool((res.energy_after[:, 3] < res.energy_before[:, 3]).all())
    assert bool((res.scores_after.total < res.scores_before.total).all())
    assert bool((res.accepted >= 1).all()) and res.accepted.dtype == torch.int32
    bonds, _ = R.ligand_torsions(g)
    worst = 0.0
    for frag in rigid_fragments(37, g["ligand", "ligand"].edge_index.numpy(), bonds):
        if len(frag) > 1:
            d0, d1 = torch.cdist(x0[:, frag].double(), x0[:, frag].double()), torch.cdist(res.lig_pos[:, frag].double(), res.lig_pos[:, frag].double())
            worst = max(worst, float((d0 - d1).abs().max()))
    assert worst <= 1e-4, worst
    crystal = g["ligand"].pos.float()[None]
    before, after = plain_rmsd(x0, crystal), plain_rmsd(res.lig_pos, crystal)
    print(f"{what}: E {float(res.energy_before[:, 3].min()):.2f} .. {float(res.energy_before[:, 3].max()):.2f} -> "
          f"{float(res.energy_after[:, 3].max()):.2f} .. {float(res.energy_after[:, 3].min()):.2f}; total "
          f"{float(res.scores_before.total.min()):.2f} .. {float(res.scores_before.total.max()):.2f} -> "
          f"{float(res.scores_after.total.max()):.2f} .. {float(res.scores_after.total.min()):.2f}; median RMSD to the crystal pose "
          f"{float(before.median()):.3f} -> {float(after.median()):.3f}; moved {float(res.rmsd_moved.min()):.2f} .. "
          f"{float(res.rmsd_moved.max()):.2f}; accepted {int(res.accepted.min())} .. {int(res.accepted.max())}; fragment distances "
          f"off by {worst:.2e}")
    assert float(after.median()) < 0.75 * float(before.median())
    assert torch.allclose(res.rmsd_moved.double(), plain_rmsd(res.lig_pos, x0), atol=1e-5)


def chain_case(S, n, T, m, seed):
    """A hand-made ligand for the raw entry: a random-walk chain of n atoms (1.5 A steps), T rotatable bonds (a, a + 1), a = 1, 3, ...,
    each turning the atoms behind it; typed atoms, flags and a crowded random receptor as vinardo_ref.random_case draws them.
    Returns (x [S, n, 3], lig_r, lig_f, rec [m, 3], rec_r, rec_f, pairs, bonds int32 [T, 2], mask uint8 [T, n]) as host tensors."""
    (x, lig_r, lig_f, rec, rec_r, rec_f, pairs), _ = as_torch(V.random_case(S, n, m, seed))
    gen = torch.Generator().manual_seed(seed)
    steps = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1) * 1.5
    chain = torch.cumsum(steps, 0)
    chain = chain - chain.mean(0, keepdim=True)
    x = (chain[None] + 0.05 * torch.randn(S, n, 3, generator=gen)).float().contiguous()
    rec = (rec * 0.6).contiguous()                          # around the chain
    assert 2 * T < n
    bonds = torch.tensor([[2 * j + 2, 2 * j + 1] for j in range(T)], dtype=torch.int32).reshape(T, 2)
    mask = torch.zeros(T, n, dtype=torch.uint8)
    for j in range(T):
        mask[j, 2 * j + 2:] = 1
    return x, lig_r, lig_f, rec, rec_r, rec_f, pairs, bonds, mask


def tiled_graph(copies):
    """The 3dpf complex with its ligand repeated `copies` times (3 A apart along x): a ligand above the fused kernel's atom limit,
    with only the fields a PoseMinimizer reads."""
    g, _, _ = fixture_3dpf()
    n = g["ligand"].pos.shape[0]
    bonds_mask = g["ligand"].mask_rotate
    mr = torch.as_tensor(np.asarray(bonds_mask if isinstance(bonds_mask, np.ndarray) else bonds_mask[0])).bool()
    T = mr.shape[0]
    big = HeteroBatch()
    shift = torch.tensor([3.0, 0.0, 0.0])
    big["ligand"].pos = torch.cat([g["ligand"].pos.float() + k * shift for k in range(copies)], 0)
    big["ligand"].x = g["ligand"].x.repeat(copies, 1)
    big["ligand"].edge_mask = g["ligand"].edge_mask.repeat(copies)
    mask = torch.zeros(copies * T, copies * n, dtype=torch.bool)
    for k in range(copies):
        mask[k * T:(k + 1) * T, k * n:(k + 1) * n] = mr
    big["ligand"].mask_rotate = mask.numpy()
    big["ligand", "ligand"].edge_index = torch.cat([g["ligand", "ligand"].edge_index + k * n for k in range(copies)], 1)
    big["atom"].pos = g["atom"].pos.clone()
    big["atom"].x = g["atom"].x.clone()
    return big


# ---------------------------------------------------------------------------------------------- 1. energy and gradient
@pytest.mark.parametrize("n,m", [(1, 1), (4, 7), (37, 300)])
def test_energy_is_the_score_plus_the_restraint(n, m):
    k = 0.3
    (x, lig_r, lig_f, rec, rec_r, rec_f, pairs), ref = as_torch(V.random_case(3, n, m, 900 + n + m))
    anchor = x + 0.2 * torch.randn(x.shape, generator=torch.Generator().manual_seed(n))
    e, g = M.energy_torch(x, anchor, lig_r, lig_f, rec, rec_r, rec_f, pairs, CFG, k)
    e7, g7 = SC.score_torch(x, lig_r, lig_f, rec, rec_r, rec_f, pairs, CFG, 1.7, with_grad=True)
    dx = x.double() - anchor.double()
    rest = k * dx.pow(2).sum(-1).mean(-1)
    assert e.shape == (3, 4) and e.dtype == torch.float64 and g.shape == (3, n, 3)
    assert torch.equal(e[:, 0], e7[:, 4]) and torch.equal(e[:, 1], e7[:, 5])          # not divided by the torsion divisor
    assert torch.allclose(e[:, 2], rest, rtol=1e-14, atol=0) and bool((e[:, 2] > 0).all())
    assert torch.allclose(e[:, 3], e7[:, 4] + e7[:, 5] + rest, rtol=1e-14, atol=1e-300)
    assert torch.allclose(g, g7 + (2 * k / n) * dx, rtol=1e-13, atol=1e-300)
    # and against the NumPy restatement, within its bound
    be, bg = V.bounds(ref)
    assert (np.abs(e[:, 0].numpy() - ref["energy"][:, 4]) <= be[:, 4]).all() and (np.abs(e[:, 1].numpy() - ref["energy"][:, 5]) <= be[:, 5]).all()
    assert (np.abs((g - (2 * k / n) * dx).numpy() - ref["grad"]) <= bg[:, None, None]).all()
    # k = 0: the restraint vanishes exactly
    e0, g0 = M.energy_torch(x, anchor, lig_r, lig_f, rec, rec_r, rec_f, pairs, CFG, 0.0)
    assert torch.equal(e0[:, 2], torch.zeros(3, dtype=torch.float64)) and torch.equal(g0, g7) and torch.equal(e0[:, 3], e7[:, 4] + e7[:, 5])


def test_gradient_is_the_autograd_derivative_of_the_fp64_form():
    k = 0.4
    for seed, (n, m) in enumerate(((4, 30), (37, 300))):
        (x, lig_r, lig_f, rec, rec_r, rec_f, pairs), _ = as_torch(V.random_case(2, n, m, 60 + seed))
        anchor = x + 0.3 * torch.randn(x.shape, generator=torch.Generator().manual_seed(seed))
        e, g = M.energy_torch(x, anchor, lig_r, lig_f, rec, rec_r, rec_f, pairs, CFG, k)
        x64 = x.double().requires_grad_(True)

        def energy(a, b, ra, fa, rb, fb, keep):
            d = (a[:, None] - b[None]).pow(2).sum(-1).clamp(min=1e-300).sqrt()
            s = d - (ra.double()[:, None] + rb.double()[None])
            ok = keep & (ra[:, None] >= 0) & (rb[None] >= 0) & (d < 8.0)
            fa, fb = fa.long()[:, None], fb.long()[None]
            hyd, hb = (fa & fb & 1) != 0, ((((fa >> 1) & (fb >> 2)) | ((fa >> 2) & (fb >> 1))) & 1) != 0
            t = -0.045 * torch.exp(-(s / 0.8) ** 2) + 0.8 * torch.where(s < 0, s * s, torch.zeros_like(s))
            t = t - 0.035 * hyd.double() * (1 - s / 2.5).clamp(0, 1) - 0.6 * hb.double() * (-s / 0.6).clamp(0, 1)
            return torch.where(ok, t, torch.zeros_like(t)).sum()

        sym = (pairs.bool() | pairs.bool().T)
        total = sum(energy(x64[s], rec.double(), lig_r, lig_f, rec_r, rec_f, torch.ones(n, m, dtype=torch.bool))
                    + 0.5 * energy(x64[s], x64[s], lig_r, lig_f, lig_r, lig_f, sym)
                    + k * (x64[s] - anchor[s].double()).pow(2).sum(-1).mean() for s in range(2))
        want, = torch.autograd.grad(total, x64)
        scale = float(want.abs().max())
        assert scale > 0 and float((g - want).abs().max()) <= 1e-10 * scale, float((g - want).abs().max()) / scale
        assert abs(float(total.detach()) - float(e[:, 3].sum())) <= 1e-10 * abs(float(total.detach()))


# ---------------------------------------------------------------------------------------------- 2. invariants of a run
def test_a_run_on_the_fixture_descends_and_keeps_the_fragments_rigid():
    res, hist = run_50()
    x0 = perturbed_poses()
    before = x0.clone()
    check_invariants(res, hist, x0, "CPU form, 50 iterations")
    assert torch.equal(x0, before), "the input tensor was modified"
    assert res.lig_pos.dtype == torch.float32 and res.energy_before.shape == (16, 4) and res.energy_after.dtype == torch.float64
    assert isinstance(res.scores_after, SC.PoseScores) and isinstance(res.cpu(), M.MinimizeResult)
    # energy_* are E's parts: inter and intra as the scorer reports them, undivided
    assert torch.equal(res.energy_after[:, 0], res.scores_after.inter) and torch.equal(res.energy_after[:, 1], res.scores_after.intra)
    assert torch.equal(res.energy_after[:, 2], torch.zeros(16, dtype=torch.float64))
    assert torch.equal(res.energy_after[:, 3], res.energy_after[:, 0] + res.energy_after[:, 1])


def test_advance_resumes_a_run():
    g, _, full = fixture_3dpf()
    mz = M.PoseMinimizer(g, receptor=full)
    x0 = perturbed_poses()[:3]
    step, acc = torch.ones(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32)
    whole = mz.advance(x0, x0, step, acc, 7)
    x, s, a, e_in, _ = mz.advance(x0, x0, step, acc, 3)
    part = mz.advance(x, x0, s, a, 4)
    assert torch.equal(bits32(whole[0]), bits32(part[0])) and torch.equal(whole[1], part[1]) and torch.equal(whole[2], part[2])
    assert torch.equal(whole[4], part[4]) and torch.equal(whole[3], e_in)
    assert torch.equal(step, torch.ones(3, dtype=torch.float64)) and int(acc.sum()) == 0      # the arguments are not modified


# ---------------------------------------------------------------------------------------------- 3. the restraint
def test_the_restraint_holds_the_poses_back():
    free, _ = run_50()
    g, _, full = fixture_3dpf()
    held = M.PoseMinimizer(g, receptor=full, config=M.MinimizeConfig(iterations=50, restraint=0.5)).minimize(perturbed_poses())
    print("rmsd_moved, k = 0:", [round(float(v), 3) for v in free.rmsd_moved], "k = 0.5:", [round(float(v), 3) for v in held.rmsd_moved])
    assert bool((held.rmsd_moved <= free.rmsd_moved + 0.05).all())
    assert bool((held.energy_after[:, 2] > 0).all()) and torch.equal(held.energy_before[:, 2], torch.zeros(16, dtype=torch.float64))
    assert bool((held.energy_after[:, 3] < held.energy_before[:, 3]).all())
    with pytest.raises(ValueError):
        M.PoseMinimizer(g, config=M.MinimizeConfig(restraint=-1.0))
    with pytest.raises(ValueError):
        M.PoseMinimizer(g, config=M.MinimizeConfig(iterations=-1))


# ---------------------------------------------------------------------------------------------- 4. NaN, iterations = 0, shapes
def test_a_nan_pose_is_kept_bit_for_bit_and_touches_no_other_sample():
    g, _, full = fixture_3dpf()
    mz = M.PoseMinimizer(g, receptor=full, config=M.MinimizeConfig(iterations=6))
    x = perturbed_poses()[:4]
    clean = mz.minimize(x)
    bad = x.clone()
    bad[2, 5, 1] = float("nan")
    got = mz.minimize(bad)
    assert torch.equal(bits32(got.lig_pos[2]), bits32(bad[2])) and int(got.accepted[2]) == 0
    assert bool(torch.isnan(got.energy_before[2, 3])) and bool(torch.isnan(got.energy_after[2, 3]))
    for s in (0, 1, 3):
        assert torch.equal(bits32(got.lig_pos[s]), bits32(clean.lig_pos[s])) and torch.equal(got.energy_after[s], clean.energy_after[s])
        assert int(got.accepted[s]) == int(clean.accepted[s]) >= 1


def test_zero_iterations_and_zero_samples_are_the_identity():
    g, _, full = fixture_3dpf()
    mz = M.PoseMinimizer(g, receptor=full, config=M.MinimizeConfig(iterations=0))
    x = perturbed_poses()[:3]
    h = []
    got = mz.minimize(x, history=h)
    assert torch.equal(bits32(got.lig_pos), bits32(x)) and got.lig_pos.data_ptr() != x.data_ptr()
    assert torch.equal(got.energy_before, got.energy_after) and len(h) == 1 and torch.equal(h[0], got.energy_before[:, 3])
    assert int(got.accepted.sum()) == 0 and float(got.rmsd_moved.max()) == 0.0
    e, grad = mz.energy(x)
    assert torch.equal(e, got.energy_before) and grad.shape == (3, 37, 3)
    empty = M.PoseMinimizer(g, receptor=full, config=M.MinimizeConfig(iterations=2)).minimize(x[:0])
    assert empty.lig_pos.shape == (0, 37, 3) and empty.energy_after.shape == (0, 4) and empty.scores_after.total.shape == (0,)
    with pytest.raises(ValueError):
        mz.minimize(x[:, :5])
    with pytest.raises(ValueError):
        mz.minimize(x, atom_pos=torch.zeros(2, mz.n_a, 3))
    import diffdock_pocket_amd as DP
    assert DP.PoseMinimizer is M.PoseMinimizer and DP.MinimizeConfig is M.MinimizeConfig and DP.MinimizeResult is M.MinimizeResult
    c = M.MinimizeConfig()
    assert (c.iterations, c.restraint, c.step_init, c.step_grow, c.step_shrink, c.step_max) == (100, 0.0, 1.0, 2.0, 0.5, 1024.0)


def flexible_case():
    """(graph, poses [3, 12, 3], atom_pos [3, n_a, 3], the typed receptor atom nearest to the ligand) of the flexible synthetic graph."""
    g = make_3dpf_complex(flexible_sidechains=True, n_lig=12, n_rec=8)
    gen = torch.Generator().manual_seed(5)
    lig = (g["ligand"].pos.float()[None] + 0.3 * torch.randn(3, 12, 3, generator=gen)).contiguous()
    apos = g["atom"].pos.float()[None].repeat(3, 1, 1).contiguous()
    typed = torch.nonzero(SC.PoseScorer(g)._cpu["rec_r"] >= 0).reshape(-1)
    d = torch.cdist(lig[1].double(), apos[1, typed].double()).min(0).values
    assert float(d.min()) < 8.0
    return g, lig, apos, int(typed[int(d.argmin())])


def test_flexible_graph_minimises_each_sample_against_its_own_atoms():
    g, lig, apos, row = flexible_case()
    mz = M.PoseMinimizer(g, config=M.MinimizeConfig(iterations=5))
    base = mz.minimize(lig, atom_pos=apos)
    assert torch.equal(bits32(base.lig_pos), bits32(mz.minimize(lig).lig_pos))          # the graph's own atoms, replicated
    moved = apos.clone()
    moved[1, row] += 30.0
    got = mz.minimize(lig, atom_pos=moved)
    for s in (0, 2):
        assert torch.equal(bits32(got.lig_pos[s]), bits32(base.lig_pos[s])) and torch.equal(got.energy_after[s], base.energy_after[s])
    assert not torch.equal(got.energy_before[1], base.energy_before[1])


# ---------------------------------------------------------------------------------------------- 5. ABI
def test_entry_is_declared_exported_built_and_guarded():
    header = open(os.path.join(ROOT, "include", "ddp_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(ddp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert "ddp_pose_minimize" in declared and "ddp_pose_minimize" in L.EXPORTS and set(L.EXPORTS) == declared
    assert "#define DDP_ABI_VERSION 17" in header and "ddp_minimize_args_t" in header
    assert f"#define DDP_MINIMIZE_MAX_ATOMS {L.DDP_MINIMIZE_MAX_ATOMS}" in header and L.DDP_MINIMIZE_MAX_ATOMS >= 256
    assert f"#define DDP_MINIMIZE_MAX_TORSIONS {L.DDP_MINIMIZE_MAX_TORSIONS}" in header
    assert "ddp_minimize.hip" in __import__("diffdock_pocket_amd.build", fromlist=["SOURCES"]).SOURCES
    assert os.path.exists(L.LIB_PATH), "build the library first (python -m diffdock_pocket_amd.build)"
    lib = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(lib, "ddp_pose_minimize")
    lib.ddp_abi_version.restype = ctypes.c_int
    assert lib.ddp_abi_version() == 17
    # the ctypes mirror has the size the header's struct has on this ABI: 6 int32, 10 pointers, 15 doubles, 6 pointers
    assert ctypes.sizeof(L.MinimizeArgs) == 24 + 10 * 8 + 15 * 8 + 6 * 8
    body = header[header.index("typedef struct {", header.index("DDP_MINIMIZE_MAX_TORSIONS 4096")):header.index("} ddp_minimize_args_t;")]
    fields = re.findall(r"([a-z_0-9]+)(?=\s*[,;])", re.sub(r"/\*.*?\*/", "", body))
    assert fields == [f[0] for f in L.MinimizeArgs._fields_], fields
    # the host-side checks of the entry need no device: they return before any launch
    lib.ddp_pose_minimize.argtypes, lib.ddp_pose_minimize.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    assert lib.ddp_pose_minimize(None, None) == -1
    assert lib.ddp_pose_minimize(ctypes.byref(L.MinimizeArgs(n_samples=0)), None) == 0
    assert lib.ddp_pose_minimize(ctypes.byref(L.MinimizeArgs(n_samples=1, n=L.DDP_MINIMIZE_MAX_ATOMS + 1, m=0)), None) == -2
    assert lib.ddp_pose_minimize(ctypes.byref(L.MinimizeArgs(n_samples=1, n=4, m=0, n_tor=L.DDP_MINIMIZE_MAX_TORSIONS + 1)), None) == -2
    assert lib.ddp_pose_minimize(ctypes.byref(L.MinimizeArgs(n_samples=1, n=4, m=0)), None) == -1          # null pointers
    assert lib.ddp_pose_minimize(ctypes.byref(L.MinimizeArgs(n_samples=-1, n=4, m=0)), None) == -1


# ---------------------------------------------------------------------------------------------- 6. flags and driver
def test_flags_parse_and_default_to_off(tmp_path, capsys):
    p = INF._parser()
    a = p.parse_args([])
    assert a.minimize_poses is False and a.rank_by == "confidence" and a.minimize_iterations == 100 and a.minimize_restraint == 0.0
    a = p.parse_args(["--minimize_poses", "--minimize_iterations", "7", "--minimize_restraint", "0.25", "--rank_by", "minimized_score"])
    assert a.minimize_poses is True and a.minimize_iterations == 7 and a.minimize_restraint == 0.25 and a.rank_by == "minimized_score"
    (tmp_path / "model_parameters.yml").write_text("{}\n")
    for bad in (["--minimize_iterations", "-1"], ["--minimize_restraint", "-0.5"]):
        with pytest.raises(SystemExit) as e:
            INF.main(["--protein_path", "p.pdb", "--ligand", "l.sdf", "--model_dir", str(tmp_path)] + bad)
        assert e.value.code == 2 and "--minimize_iterations and --minimize_restraint must not be negative" in capsys.readouterr().err
    with pytest.raises(ValueError, match="rank_by"):
        INF.run_csv("none.csv", None, torch.device("cpu"), rank_by="minimised")


def test_run_csv_minimises_poses_and_leaves_everything_else_alone(tmp_path):
    p = tmp_path / "complexes.csv"
    p.write_text(CSV)
    plain = _run(str(p), str(tmp_path / "plain"))
    mini = _run(str(p), str(tmp_path / "mini"), minimize_poses=M.MinimizeConfig(iterations=3))
    g, pdb, full = fixture_3dpf()
    assert len(mini) == 2
    for a, b in zip(plain, mini):
        assert a.skipped is None and b.skipped is None and a.minimized is None and a.minimized_pos is None and b.scores is None
        assert torch.equal(a.ligand_pos, b.ligand_pos) and torch.equal(a.confidence, b.confidence) and torch.equal(a.order, b.order)
        old = {os.path.basename(f): f for f in a.files}
        new = {os.path.basename(f): f for f in b.files}
        assert set(new) - set(old) == {"minimized.csv"} | {f"rank{k}_minimized.sdf" for k in range(1, 5)} and set(old) <= set(new)
        assert set(os.listdir(os.path.dirname(b.files[0]))) == set(new) and set(os.listdir(os.path.dirname(a.files[0]))) == set(old)
        for name, path in old.items():
            assert open(path, "rb").read() == open(new[name], "rb").read(), name
        mr = b.minimized
        assert isinstance(mr, M.MinimizeResult) and not mr.lig_pos.is_cuda and mr.lig_pos.shape == b.ligand_pos.shape
        assert torch.equal(mr.lig_pos, b.minimized_pos) and bool((mr.energy_after[:, 3] <= mr.energy_before[:, 3]).all())
        rows = _rows(new["minimized.csv"])
        assert O.MINIMIZED_COLUMNS == ["rank", "sample", "total_before", "total_after", "energy_before", "energy_after", "inter_after",
                                       "intra_after", "restraint_after", "rmsd_moved", "accepted_steps"]
        assert list(rows[0].keys()) == O.MINIMIZED_COLUMNS and len(rows) == 4
        for r, row in enumerate(rows):
            assert int(row["rank"]) == r + 1 and int(row["sample"]) == int(b.order[r]) and int(row["accepted_steps"]) == int(mr.accepted[r])
            for col, val in (("total_before", mr.scores_before.total[r]), ("total_after", mr.scores_after.total[r]),
                             ("energy_before", mr.energy_before[r, 3]), ("energy_after", mr.energy_after[r, 3]),
                             ("inter_after", mr.energy_after[r, 0]), ("intra_after", mr.energy_after[r, 1]),
                             ("restraint_after", mr.energy_after[r, 2])):
                assert abs(float(row[col]) - float(val)) <= 1e-5 * abs(float(val)) + 1e-12, col
            assert abs(float(row["rmsd_moved"]) - float(mr.rmsd_moved[r])) < 1e-4
        from diffdock_pocket_amd import inputs as I
        for r in range(4):
            got = I.ligand_graph(I.parse_sdf(open(new[f"rank{r + 1}_minimized.sdf"]).read()))[1] - np.asarray(b.original_center, dtype=np.float64).reshape(1, 3)
            assert np.abs(got - mr.lig_pos[r].double().numpy()).max() < 2e-4
    # the rigid row ran against the full typed PDB, from the sampled poses, in this package's CPU form
    want = M.PoseMinimizer(g, receptor=full, config=M.MinimizeConfig(iterations=3)).minimize(mini[1].ligand_pos)
    assert torch.equal(bits32(want.lig_pos), bits32(mini[1].minimized_pos)) and torch.equal(want.energy_after, mini[1].minimized.energy_after)
    assert torch.equal(want.scores_before.total, SC.PoseScorer(g, receptor=full).score(mini[1].ligand_pos).total)


def test_rank_by_minimized_score_reorders_everything_downstream(tmp_path):
    p = tmp_path / "complexes.csv"
    p.write_text(CSV)
    by_conf = _run(str(p), str(tmp_path / "conf"), minimize_poses=M.MinimizeConfig(iterations=3), score_poses=SC.ScoreConfig())
    by_min = _run(str(p), str(tmp_path / "min"), rank_by="minimized_score", score_poses=SC.ScoreConfig())      # implies minimisation
    assert by_min[0].minimized is not None
    again = _run(str(p), str(tmp_path / "min3"), rank_by="minimized_score", minimize_poses=M.MinimizeConfig(iterations=3),
                 score_poses=SC.ScoreConfig())
    for a, b in zip(by_conf, again):
        assert b.skipped is None
        t = b.minimized.scores_after.total
        assert bool((t[:-1] <= t[1:]).all()) and sorted(b.order.tolist()) == [0, 1, 2, 3]
        inv_a, inv_b = torch.argsort(a.order), torch.argsort(b.order)
        assert torch.equal(a.ligand_pos[inv_a], b.ligand_pos[inv_b]) and torch.equal(a.scores.total[inv_a], b.scores.total[inv_b])
        assert torch.equal(bits32(a.minimized_pos[inv_a]), bits32(b.minimized_pos[inv_b]))
        assert b.order.tolist() == SC.rank_order(a.minimized.scores_after.total[inv_a]).tolist()
        files = {os.path.basename(f): f for f in b.files}
        assert [int(r["sample"]) for r in _rows(files["minimized.csv"])] == b.order.tolist()
        assert [int(r["sample"]) for r in _rows(files["scores.csv"])] == b.order.tolist()
        assert [int(r["sample"]) for r in _rows(files["modes.csv"])] == b.order.tolist()
        assert int(b.clusters.labels[0]) == 0
