"""python tools/descent_bits.py [out.json]  (needs an MI355X; profiles/descent_bits.json, profiles/pose_family_bits.json and
profiles/pose_family_loop_bits.json)
SHA-256 of every output tensor's bytes of the entries that share csrc/ddp_pose_descent.h and csrc/ddp_horn.h, and of the rest of the
pose family (ddp_pose_profile, ddp_pose_minimize_flex, ddp_clash_guidance, ddp_pose_search, ddp_pose_search_select,
ddp_pose_search_flex, ddp_score_guidance, ddp_score_guidance_flex with every intermediate state and the start poses), on seeded inputs
only: the 3dpf fixture of tests/golden, synthetic ragged shapes, the small cases of tests/pose_form_cases.py at the default and at a
non-default score form, and the small shapes of the searches' and the guidance terms' GPU tests through those tests' own launch
helpers.  Run once per library (DDP_HIP_LIB selects one) in a fresh process; two libraries compute the same bits iff their digest
lists are equal."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pose_form_cases as P       # NumPy only: the seeded inputs of tests/test_gpu_pose_form.py
from diffdock_pocket_amd import guidance as G
from diffdock_pocket_amd import inputs as I
from diffdock_pocket_amd import launch as LA
from diffdock_pocket_amd import minimize as M
from diffdock_pocket_amd import refine as R
from diffdock_pocket_amd import scoring as SC
from diffdock_pocket_amd.sampler import apply_sidechain_torsions_hip, modify_conformer, modify_conformer_hip

dev = torch.device("cuda:0")
out = {}


def put(name, *tensors):
    for k, t in enumerate(tensors):
        out[f"{name}[{k}]"] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def synthetic(S, n, m, T, seed, per_sample):
    """A random-walk chain of n atoms with T rotatable bonds (2 j + 2, 2 j + 1) that turn the atoms behind them, a crowded receptor of m
    atoms, radii with untyped atoms (-1) on both sides, every flag byte, random self pairs; device tensors."""
    rng = np.random.default_rng(seed)
    steps = rng.standard_normal((n, 3))
    chain = np.cumsum(1.5 * steps / np.linalg.norm(steps, axis=1, keepdims=True), 0)
    x = (chain - chain.mean(0) + 0.05 * rng.standard_normal((S, n, 3))).astype(np.float32)
    box = 1.2 * max(n, 8) ** (1 / 3)
    rec = (rng.standard_normal((S, m, 3) if per_sample else (m, 3)) * box).astype(np.float32)
    table = np.array([1.9, 1.8, 1.7, 2.0, 1.5, -1.0], dtype=np.float32)
    c = dict(x=x, anchor=x + 0.1 * rng.standard_normal(x.shape).astype(np.float32), lig_r=table[rng.integers(0, 6, n)],
             rec=rec, rec_r=table[rng.integers(0, 6, m)], lig_f=rng.integers(0, 8, n).astype(np.uint8),
             rec_f=rng.integers(0, 8, m).astype(np.uint8), pairs=np.triu(rng.random((n, n)) < 0.5, 1).astype(np.uint8),
             bonds=np.array([[2 * j + 2, 2 * j + 1] for j in range(T)], dtype=np.int32).reshape(T, 2),
             mask=np.array([[i >= 2 * j + 2 for i in range(n)] for j in range(T)], dtype=np.uint8).reshape(T, n),
             step=2.0 ** rng.integers(-3, 4, S).astype(np.float64))
    return {k: torch.from_numpy(v).to(dev) for k, v in c.items()}


f64 = dict(dtype=torch.float64, device=dev)
for S, n, m, T, per_sample in ((3, 1, 0, 0, False), (3, 5, 1, 1, False), (2, 37, 1025, 5, True), (3, 130, 300, 7, False), (2, 256, 2085, 5, False)):
    c = synthetic(S, n, m, T, 1000 + n + m, per_sample)
    tag = f"S{S}_n{n}_m{m}_T{T}"
    # ddp_refine_energy, ddp_refine_direction (the clash radii: untyped receptor atoms are the hydrogens, ligand radii positive)
    e, g = torch.empty(S, 4, **f64), torch.empty(S, n, 3, **f64)
    tr, rot, tor = torch.empty(S, 3, device=dev), torch.empty(S, 3, device=dev), torch.empty(S, T, device=dev)
    a = LA.refine_args(c["x"], c["anchor"], c["lig_r"].abs(), c["rec"], c["rec_r"], c["pairs"], 0.4, 0.1, e, g, bonds=c["bonds"],
                       mask_rotate=c["mask"], step=c["step"], tr=tr, rot=rot, tor=tor)
    LA.refine_energy(a)
    LA.refine_direction(a)
    put(f"refine_energy_direction {tag}", e, g, tr, rot, tor)
    # ddp_pose_update with and without torsions, on the steps just computed and on larger ones
    for scale in (1.0, 40.0):
        put(f"pose_update {tag} x{scale}", modify_conformer_hip(c["x"], scale * tr, scale * rot, scale * tor if T else None, c["bonds"], c["mask"]),
            modify_conformer_hip(c["x"], scale * tr, scale * rot, None, None, None))
    # ddp_pose_score, both variants
    args = (c["x"], c["lig_r"], c["lig_f"], c["rec"], c["rec_r"], c["rec_f"], SC.ScoreConfig())
    for pairs in (c["pairs"], None):
        put(f"pose_score {tag} pairs={pairs is not None}", *LA.pose_score(*args, 1.7, pairs, with_grad=True), LA.pose_score(*args, 1.7, pairs)[0])
    # ddp_pose_minimize
    for iterations in (0, 1, 12):
        for Tm in sorted({0, min(T, 1), min(T, 5)}):
            for k in (0.0, 0.3):
                x, step, acc = c["x"].clone(), c["step"].clone(), torch.zeros(S, dtype=torch.int32, device=dev)
                e0, e1, h, gm = torch.empty(S, 4, **f64), torch.empty(S, 4, **f64), torch.empty(iterations + 1, S, **f64), torch.empty(S, n, 3, **f64)
                LA.pose_minimize(x, c["anchor"], c["lig_r"], c["lig_f"], c["rec"], c["rec_r"], c["rec_f"], SC.ScoreConfig(), c["pairs"],
                                 c["bonds"][:Tm].contiguous() if Tm else None, c["mask"][:Tm].contiguous() if Tm else None, step, acc, e0, e1,
                                 iterations, restraint=k, history=h, grad=gm)
                put(f"pose_minimize {tag} it={iterations} T={Tm} k={k}", x, step, acc, e0, e1, h, gm)

# ---- the rest of the pose family, at the default form and at the non-default one of the tests
forms = {"default": SC.ScoreConfig(), "form": SC.ScoreConfig(**P.FORM)}
dv = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).to(dev)
# ddp_pose_profile: residues of 0, 1, 12 and 65 atoms, a ligand inside one wave's lanes and one beyond them
for n in (37, 70):
    x, lig_r, lig_f, rec, rec_r, rec_f, ptr = (dv(a) for a in P.profile_case(n)[:7])
    for tag, cfg in forms.items():
        put(f"pose_profile n{n} {tag}", *LA.pose_profile(x, lig_r, lig_f, rec, rec_r, rec_f, ptr, cfg, 4.5))
# ddp_pose_minimize_flex: S = 2, n = 37, m = 70, 9 moving atoms, 3 side-chain bonds
fc = P.flex_case()
ft = {k: dv(fc[k]) for k in ("x", "y", "x0", "y0", "lig_r", "lig_f", "rec_r", "rec_f", "pairs")}


class _Tables:
    mov, pairs, edge_idx, mapping, sub = (torch.from_numpy(fc[k]) for k in ("mov", "sc_pairs", "edge", "mapping", "sub"))


tables = LA.flex_tables(_Tables, fc["y"].shape[1], dev)
for tag, cfg in forms.items():
    for iterations in (0, 1, 12):
        S, n = fc["x"].shape[:2]
        x, y, step, acc = ft["x"].clone(), ft["y"].clone(), torch.ones(S, **f64), torch.zeros(S, dtype=torch.int32, device=dev)
        e0, e1, h = torch.empty(S, 6, **f64), torch.empty(S, 6, **f64), torch.empty(iterations + 1, S, **f64)
        gx, gy = torch.empty(S, n, 3, **f64), torch.empty(S, len(fc["mov"]), 3, **f64)
        LA.pose_minimize_flex(x, ft["x0"], ft["lig_r"], ft["lig_f"], y, ft["y0"], ft["rec_r"], ft["rec_f"], cfg, ft["pairs"], None, None, tables,
                              step, acc, e0, e1, iterations, restraint=fc["k"], restraint_sc=fc["k_sc"], history=h, grad=gx, grad_mov=gy)
        put(f"pose_minimize_flex {tag} it={iterations}", x, y, step, acc, e0, e1, h, gx, gy)
# ddp_clash_guidance (no score form: the shared host checks only): S = 2, n = 37, m = 1025, 5 torsions, shared and per-sample receptor
c = synthetic(2, 37, 1025, 5, 2087, True)
gt = G.GuidanceTables(c["lig_r"].abs().cpu(), c["rec"][0].cpu(), c["rec_r"].cpu(), c["pairs"].cpu(), c["bonds"].cpu().long(), c["mask"].cpu().bool())
ws = G.GuidanceWorkspace(gt, dev)
weight = torch.tensor([0.75], dtype=torch.float32, device=dev)
for rec in (None, c["rec"]):
    upd = (torch.full((2, 3), 0.125, device=dev), torch.full((2, 3), -0.25, device=dev), torch.full((2, 5), 0.5, device=dev))
    ge, gg = torch.empty(2, 2, **f64), torch.empty(2, 37, 3, **f64)
    ws.launch(c["x"], rec, upd, weight, ge, gg)
    put(f"clash_guidance per_sample={rec is not None}", *upd, ge, gg)

# ddp_sidechain_update: two bonds, the second turning a subset of the first's atoms
gen = torch.Generator().manual_seed(3)
pos = torch.randn(3, 40, 3, generator=gen).to(dev)
edge = torch.tensor([[1, 0], [5, 4]], dtype=torch.int32, device=dev)
sub = torch.tensor(list(range(2, 12)) + list(range(6, 12)), dtype=torch.int32, device=dev)
mp = torch.tensor([[0, 10], [10, 16]], dtype=torch.int32, device=dev)
put("sidechain_update", apply_sidechain_torsions_hip(pos, edge, sub, mp, torch.randn(3, 2, generator=gen).to(dev)))

# the two drivers on 16 perturbed poses of the fixture (the perturbation recipe of the test fixtures)
GOLDEN = os.path.join(ROOT, "tests", "golden")
pdb, sdf = open(os.path.join(GOLDEN, "3dpf_protein.pdb")).read(), open(os.path.join(GOLDEN, "3dpf_ligand.sdf")).read()
g = I.build_complex_graph(pdb, sdf)
host = M.PoseMinimizer(g, receptor=SC.typed_receptor(pdb, g.original_center))
gen = torch.Generator().manual_seed(2)
tr = torch.randn(16, 3, generator=gen, dtype=torch.float64) * 0.5
rot = torch.randn(16, 3, generator=gen, dtype=torch.float64) * 0.15
tor = torch.randn(16, host.T, generator=gen, dtype=torch.float64) * 0.3
xd = modify_conformer(g["ligand"].pos.float()[None].expand(16, -1, -1).contiguous(), tr.float(), rot.float(), tor.float(), host.bonds,
                      host.rot_idx).contiguous().to(dev)
h = []
r = R.PoseRefiner(g, dev).refine(xd, history=h)
put("PoseRefiner.refine", r.lig_pos, r.energy_before, r.energy_after, r.clashes_before, r.clashes_after, r.rmsd_moved, r.accepted, torch.stack(h))
mz = M.PoseMinimizer(g, dev, receptor=SC.typed_receptor(pdb, g.original_center), config=M.MinimizeConfig(iterations=30, restraint=0.05))
for fused in (True, False):
    h = []
    r = mz.minimize(xd, history=h, fused=fused)
    put(f"PoseMinimizer.minimize fused={fused}", r.lig_pos, r.energy_before, r.energy_after, r.scores_before.terms, r.scores_before.total,
        r.scores_after.terms, r.scores_after.intra, r.scores_after.total, r.rmsd_moved, r.accepted, torch.stack(h))

# ---- the searches and the score guidance, at the small shapes and through the launch helpers of their GPU tests
import score_guidance_ref as SGR
import test_gpu_score_guidance as GSG
import test_gpu_score_guidance_flex as GSGF
import test_gpu_search as GS
import test_gpu_search_flex as GSF
from test_minimize_cpu import chain_case
from test_score_guidance_flex_cpu import CASES as FLEX_GUIDANCE_CASES, case as flex_guidance_case


def put_state(name, st):
    put(name, *(st[k] for k in sorted(st) if st[k] is not None))


# ddp_pose_search, ddp_pose_search_select: 2 poses x 3 replicas x 4 cycles x 6 iterations, whole and as 1 + 3 cycles
for n, T in ((1, 0), (12, 1), (37, 5)):
    case = [a.to(dev) for a in chain_case(2, n, T, 1025, 31 + n + T)]
    p, u = GS._numbers(4, 6, T, 7, dev)
    for k in (0.0, 0.3):
        whole = GS._search(case, 3, 6, p, u, starts=True, k=k)
        a = GS._search(case, 3, 6, p[:1], u[:1], starts=True, k=k)
        b = GS._search(case, 3, 6, p[1:], u[1:], a, cycle0=1, starts=True, k=k)
        for tag, st in (("4", whole), ("1", a), ("1+3", b)):
            put_state(f"pose_search n{n} T{T} k={k} cycles={tag}", st)
        put(f"pose_search_select n{n} T{T} k={k}", *LA.pose_search_select(whole["best_pos"], whole["best_e"], whole["best_cycle"], 3))
# ddp_pose_search_flex: the shapes of test_one_cycle_of_one_replica_is_ddp_pose_minimize_flex, 3 replicas x 4 cycles x 6 iterations
TILE = GSF.TILE
for S, n, m, n_mov, n_sc, T, seed, opt in ((3, 5, TILE - 1, 4, 1, 2, 1059, {}), (3, 37, TILE + 1, 5, 17, 5, 1093, dict(moving_at=[TILE - 1, TILE])),
                                           (3, 5, TILE - 1, 4, 0, 2, 1059, {})):
    t = GSF._case(S, n, m, n_mov, n_sc, T, seed, dev, **opt)
    p, u = GSF._numbers(4, 3 * S, T, n_sc, 7, dev)
    kw = dict(starts=True, k=0.1, k_sc=0.1)
    whole = GSF._search(t, 3, 6, p, u, **kw)
    a = GSF._search(t, 3, 6, p[:1], u[:1], **kw)
    b = GSF._search(t, 3, 6, p[1:], u[1:], a, cycle0=1, **kw)
    for tag, st in (("4", whole), ("1", a), ("1+3", b)):
        put_state(f"pose_search_flex n{n} m{m} mov{n_mov} sc{n_sc} cycles={tag}", st)
# ddp_score_guidance: shared and per-sample receptor, capped and uncapped samples in one launch (the weight of the case does that)
for n in (1, 37, 256):
    for m in (0, 1, 1025):
        for T in ((0,) if n == 1 else (0, 5)):
            for per_sample in (False, True):
                c = SGR.random_case(4, n, m, T, seed=77 + 1000 * n + m + T, per_sample_rec=per_sample, with_pairs=True)
                upd, e, g = GSG._launch(c, c["w"], c["caps"], c["upd0"])
                put(f"score_guidance n{n} m{m} T{T} per_sample={per_sample} capped={c['ref']['capped'].tolist()}", *upd, e, g)
# ddp_score_guidance_flex: the cases of its tests
for shape in FLEX_GUIDANCE_CASES:
    c = flex_guidance_case(shape)
    upd, upd_sc, e, gm, _ = GSGF._launch(c, c["w"])
    put(f"score_guidance_flex {shape}", *upd, upd_sc, e, gm)
torch.cuda.synchronize()
dst = sys.argv[1] if len(sys.argv) > 1 else "descent_bits.json"
with open(dst, "w") as f:
    json.dump({"device": torch.cuda.get_device_name(0), "library": os.path.basename(os.environ.get("DDP_HIP_LIB", "libddp_hip.so")), "sha256": out}, f, indent=1)
print(len(out), "digests ->", dst)
