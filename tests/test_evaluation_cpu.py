"""Pose evaluation on the CPU (diffdock_pocket_amd/evaluation.py; reference evaluate_files.py:151-340, utils/utils.py:116-130,
datasets/steric_clash.py:99-136): graph automorphisms, the PyTorch form against a float64 NumPy restatement, properties of the
metrics, the csv driver's evaluate=True with a stub model, summarize, and the two C-ABI exports."""
import os
import re

import numpy as np
import pytest
import torch

from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import evaluation as E
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import inputs as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _edges(bonds):
    return np.array([[a for a, b in bonds] + [b for a, b in bonds], [b for a, b in bonds] + [a for a, b in bonds]])


def benzene():
    return [6] * 6, _edges([(i, (i + 1) % 6) for i in range(6)])


def neopentane():
    return [6] * 5, _edges([(0, 1), (0, 2), (0, 3), (0, 4)])


def tris_cf3_benzene():
    """1,3,5-tris(trifluoromethyl)benzene, heavy atoms: 6 ring C, 3 CF3 C, 9 F; 6 ring symmetries x (3!)^3 = 1296 automorphisms."""
    bonds, z, n = [(i, (i + 1) % 6) for i in range(6)], [6] * 6, 6
    for r in (0, 2, 4):
        c = n
        bonds.append((r, c))
        z.append(6)
        n += 1
        for _ in range(3):
            bonds.append((c, n))
            z.append(9)
            n += 1
    return z, _edges(bonds)


def graph_3dpf(flex=None):
    pdb, sdf = open(os.path.join(GOLDEN, "3dpf_protein.pdb")).read(), open(os.path.join(GOLDEN, "3dpf_ligand.sdf")).read()
    return I.build_complex_graph(pdb, sdf, flexible_sidechains=flex), pdb


def ligand_3dpf():
    g, _ = graph_3dpf()
    return (g["ligand"].x[:, 0] + 1).tolist(), g["ligand", "ligand"].edge_index.numpy()


# ---------------------------------------------------------------------------------------------- float64 restatement
def np_rmsd(pred, ref, perms):
    d = pred[:, None, :, :] - ref[perms][None]                      # [S, P, n, 3]
    v = np.sqrt((d ** 2).sum(-1).mean(-1))
    return v.min(1), v.argmin(1), v


def np_contacts(lig, lig_r, rec, rec_r, ref_c, overlap=0.4):
    rec = np.broadcast_to(rec, (lig.shape[0],) + rec.shape[-2:]) if rec.ndim == 2 else rec
    d = np.linalg.norm(lig[:, :, None] - rec[:, None], axis=-1)         # [S, n, m]
    thr = lig_r[:, None] + rec_r[None] - 2 * overlap
    clash = (d < thr[None]) & (rec_r[None, None] >= 0)
    s = np.linalg.norm(lig[:, :, None] - lig[:, None], axis=-1)
    s = np.where(np.eye(lig.shape[1], dtype=bool)[None], np.inf, s)
    return (clash.sum((1, 2)), d.min((1, 2)), s.min((1, 2)), np.linalg.norm(lig.mean(1) - ref_c[None], axis=1), d, thr)


def check_against_numpy(got, ev, lig, apos=None, rec=None, tol=1e-5):
    """PoseMetrics (any device) against the float64 restatement of the same poses."""
    t = ev._cpu
    lig64 = lig.double().cpu().numpy()
    ref = t["ref_lig"].double().numpy()
    perms = t["perms"].long().numpy()
    want, _, v = np_rmsd(lig64, ref, perms)
    assert np.allclose(got.rmsd.cpu().double().numpy(), want, rtol=tol, atol=1e-6)
    # best_perm: checked where the runner-up is clearly worse
    bp = got.best_perm.cpu().long().numpy()
    assert np.allclose(v[np.arange(len(bp)), bp], want, rtol=tol, atol=1e-6)
    if v.shape[1] > 1:
        srt = np.sort(v, 1)
        clear = srt[:, 1] - srt[:, 0] > 1e-4
        assert (bp[clear] == v.argmin(1)[clear]).all()
    plain = np.sqrt(((lig64 - ref[None]) ** 2).sum(-1).mean(-1))
    assert np.allclose(got.rmsd_plain.cpu().double().numpy(), plain, rtol=tol, atol=1e-6)
    if rec is None:
        rec = (apos.double().cpu().numpy() if (apos is not None and ev.receptor_from_graph) else t["rec"].double().numpy())
    cl, mc, ms, cen, d, thr = np_contacts(lig64, t["lig_r"].double().numpy(), rec, t["rec_r"].double().numpy(),
                                          t["ref_centroid"].double().numpy())
    assert np.allclose(got.min_cross.cpu().double().numpy(), mc, rtol=tol, atol=1e-5)
    assert np.allclose(got.min_self.cpu().double().numpy(), ms, rtol=tol, atol=1e-5)
    assert np.allclose(got.centroid.cpu().double().numpy(), cen, rtol=tol, atol=1e-5)
    band = ((np.abs(d - thr[None]) < 1e-4) & (t["rec_r"].numpy()[None, None] >= 0)).sum((1, 2))
    assert (np.abs(got.clashes.cpu().numpy().astype(np.int64) - cl) <= band).all()
    if apos is not None and t["sc_rows"] is not None:
        rows = t["sc_rows"].long().numpy()
        a64 = apos.double().cpu().numpy()[:, rows]
        sc = np.sqrt(((a64 - t["sc_ref"].double().numpy()[None]) ** 2).sum(-1).mean(-1))
        assert np.allclose(got.sc_rmsd.cpu().double().numpy(), sc, rtol=tol, atol=1e-6)


# ---------------------------------------------------------------------------------------------- automorphisms
def _check_automorphisms(z, ei, perms):
    z = np.asarray(z)
    n = len(z)
    A = np.zeros((n, n), dtype=bool)
    A[ei[0], ei[1]] = A[ei[1], ei[0]] = True
    assert perms.dtype == np.int32 and perms.shape[1] == n
    assert (perms[0] == np.arange(n)).all()
    assert len({tuple(p) for p in perms.tolist()}) == len(perms)
    for p in perms:
        assert sorted(p.tolist()) == list(range(n))
        assert (z[p] == z).all() and (A[np.ix_(p, p)] == A).all()


@pytest.mark.parametrize("mol,count", [(ligand_3dpf, 2), (benzene, 12), (neopentane, 24), (tris_cf3_benzene, 1296)])
def test_automorphism_counts_and_validity(mol, count):
    z, ei = mol()
    perms, complete = E.ligand_automorphisms(z, ei)
    assert complete and perms.shape[0] == count
    _check_automorphisms(z, ei, perms)


@pytest.mark.parametrize("mol", [ligand_3dpf, benzene, neopentane, tris_cf3_benzene])
def test_automorphisms_equal_networkx(mol):
    nx = pytest.importorskip("networkx")
    from networkx.algorithms.isomorphism import GraphMatcher
    z, ei = mol()
    G = nx.Graph()
    G.add_nodes_from((i, {"z": int(v)}) for i, v in enumerate(z))
    G.add_edges_from(zip(ei[0].tolist(), ei[1].tolist()))
    want = {tuple(m[i] for i in range(len(z))) for m in GraphMatcher(G, G, node_match=lambda a, b: a["z"] == b["z"]).isomorphisms_iter()}
    perms, _ = E.ligand_automorphisms(z, ei)
    assert {tuple(p) for p in perms.tolist()} == want


def test_automorphism_cap_falls_back_to_identity():
    z, ei = tris_cf3_benzene()
    perms, complete = E.ligand_automorphisms(z, ei, max_count=100)
    assert not complete and perms.shape == (1, len(z)) and (perms[0] == np.arange(len(z))).all()
    g, _ = graph_3dpf()
    ev = E.PoseEvaluator(g, max_automorphisms=1)
    assert not ev.symmetry_corrected and ev.n_perms == 1
    assert not ev.evaluate(g["ligand"].pos[None].float()).symmetry_corrected


# ---------------------------------------------------------------------------------------------- PyTorch form vs float64
def perturbed(ref, S, scale=0.7, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return (ref[None] + scale * torch.randn((S,) + tuple(ref.shape), generator=gen)
            + torch.randn(S, 1, 3, generator=gen)).float().contiguous()


def test_torch_form_matches_float64_rigid_full_receptor():
    g, pdb = graph_3dpf()
    rec = E.PoseEvaluator.full_receptor(pdb, g.original_center)
    ev = E.PoseEvaluator(g, receptor=rec)
    assert ev.n_perms == 2 and len(rec[1]) == 2463
    lig = perturbed(g["ligand"].pos.float(), 7)
    got = ev.evaluate(lig)
    assert got.sc_rmsd is None and got.clashes.dtype == torch.int32
    check_against_numpy(got, ev, lig)


def test_torch_form_matches_float64_flexible_graph_receptor():
    g, _ = graph_3dpf("A:160-A:193-A:197")
    ev = E.PoseEvaluator(g)
    assert ev._cpu["sc_rows"] is not None and len(ev._cpu["sc_rows"]) > 0
    lig = perturbed(g["ligand"].pos.float(), 5, seed=1)
    apos = perturbed(g["atom"].pos.float(), 5, scale=0.3, seed=2)
    got = ev.evaluate(lig, apos)
    assert got.sc_rmsd is not None
    check_against_numpy(got, ev, lig, apos)


def test_torch_form_symmetric_ligand_with_many_automorphisms():
    """The 1296-automorphism ligand: the minimum is searched over every permutation."""
    z, ei = tris_cf3_benzene()
    gen = torch.Generator().manual_seed(3)
    ref = torch.randn(len(z), 3, generator=gen) * 2
    perms, _ = E.ligand_automorphisms(z, ei)
    pred = perturbed(ref, 6, scale=1.0)
    r, b = E._rmsd_torch(pred, ref, torch.from_numpy(perms))
    want, _, v = np_rmsd(pred.double().numpy(), ref.double().numpy(), perms.astype(np.int64))
    assert np.allclose(r.double().numpy(), want, rtol=1e-6) and np.allclose(v[np.arange(6), b.long().numpy()], want, rtol=1e-6)


# ---------------------------------------------------------------------------------------------- properties
def test_relabelled_reference_has_zero_symmetry_rmsd():
    g, _ = graph_3dpf()
    ev = E.PoseEvaluator(g)
    ref = g["ligand"].pos.float()
    p = ev._cpu["perms"][1].long()
    pose = ref[p][None].contiguous()                       # atom i of the pose sits where ref atom perm[i] is
    m = ev.evaluate(pose)
    assert float(m.rmsd[0]) == 0.0 and int(m.best_perm[0]) == 1 and float(m.rmsd_plain[0]) > 0.1


def test_translated_reference_gives_rmsd_equal_centroid_equal_shift():
    g, _ = graph_3dpf()
    ev = E.PoseEvaluator(g)
    t = torch.tensor([[0.3, -1.2, 2.0], [0.0, 0.0, 0.0], [5.0, 1.0, -0.5]])
    m = ev.evaluate(g["ligand"].pos.float()[None] + t[:, None])
    norm = t.double().norm(dim=1)
    for k in ("rmsd", "centroid", "rmsd_plain"):
        assert torch.allclose(getattr(m, k).double(), norm, atol=1e-5), k


def test_receptor_hydrogens_count_for_min_cross_only():
    g, _ = graph_3dpf()
    lig = g["ligand"].pos.float()
    probe = lig[0] + torch.tensor([0.5, 0.0, 0.0])          # 0.5 A from ligand atom 0: a clash for any heavy element
    far = lig.mean(0) + 100.0
    for el, clashes in (("H", 0), ("C", 1)):
        ev = E.PoseEvaluator(g, receptor=(torch.stack([probe, far]).numpy(), [el, "O"]))
        m = ev.evaluate(lig[None].contiguous())
        assert abs(float(m.min_cross[0]) - float((lig - probe).norm(dim=1).min())) < 1e-6
        assert int(m.clashes[0]) >= clashes and (el != "H" or int(m.clashes[0]) == 0)
    assert E.vdw_radius("C") == 1.70 and E.vdw_radius(6) == 1.70 and E.vdw_radius("Fe") == 2.0 and E.vdw_radius(119) == 2.0


# ---------------------------------------------------------------------------------------------- csv driver
def _csv(tmp_path):
    p = tmp_path / "complexes.csv"
    p.write_text(
        "complex_name,experimental_protein,ligand,pocket_center_x,pocket_center_y,pocket_center_z,flexible_sidechains\n"
        "3dpf_flex,3dpf_protein.pdb,3dpf_ligand.sdf,,,,A:160-A:193-A:197\n"
        "3dpf_smiles,3dpf_protein.pdb,COc(cc1)ccc1C#N\n"
        "3dpf_rigid,3dpf_protein.pdb,3dpf_ligand.sdf\n")
    return str(p)


def _run(csv_path, **kw):
    from test_inference_csv import Stub, StubConfidence
    return INF.run_csv(csv_path, Stub(), torch.device("cpu"), confidence_model=StubConfidence(), samples_per_complex=5,
                       inference_steps=3, root=GOLDEN, seed=2, allow_zero_esm=True, **kw)


def test_csv_run_with_evaluate_reports_ranked_metrics(tmp_path):
    csv_path = _csv(tmp_path)
    plain = _run(csv_path)
    res = _run(csv_path, evaluate=True)
    assert all(r.metrics is None for r in plain)
    assert res[1].skipped is not None and res[1].metrics is None
    metrics = []
    for r, p in ((res[0], plain[0]), (res[2], plain[2])):
        assert r.skipped is None and torch.equal(r.ligand_pos, p.ligand_pos) and torch.equal(r.confidence, p.confidence)
        m = r.metrics
        assert m.rmsd.shape == (5,) and m.clashes.shape == (5,) and m.symmetry_corrected
        g, pdb = graph_3dpf(r.name == "3dpf_flex" and "A:160-A:193-A:197" or None)
        if r.name == "3dpf_flex":
            ev = E.PoseEvaluator(g)
            assert m.sc_rmsd is not None and m.sc_rmsd.shape == (5,)
            assert (m.sc_rmsd > 0).all()           # the stub turns the side chains
        else:
            ev = E.PoseEvaluator(g, receptor=E.PoseEvaluator.full_receptor(pdb, g.original_center))
            assert m.sc_rmsd is None
            want = ev.evaluate(r.ligand_pos)        # ranked order: metrics row k belongs to ligand_pos row k
            for k in ("rmsd", "centroid", "min_cross", "min_self", "clashes"):
                assert torch.equal(getattr(m, k), getattr(want, k)), k
            check_against_numpy(m, ev, r.ligand_pos)
        metrics.append(m)
    s = E.summarize(metrics)
    rm = np.stack([m.rmsd.double().numpy() for m in metrics])
    ce = np.stack([m.centroid.double().numpy() for m in metrics])
    mc = np.stack([m.min_cross.double().numpy() for m in metrics])
    cl = np.stack([m.clashes.double().numpy() for m in metrics])
    assert s["top1_rmsds_below_2"] == round(100 * float((rm[:, 0] < 2).mean()), 2)
    assert s["top1_rmsds_below_5"] == round(100 * float((rm[:, 0] < 5).mean()), 2)
    assert s["top1_mean_rmsd"] == round(float(rm[:, 0].mean()), 2)
    assert s["top1_rmsds_percentile_50"] == round(float(np.percentile(rm[:, 0], 50)), 2)
    assert s["rmsds_below_2"] == round(100 * float((rm < 2).mean()), 2)
    assert s["top5_rmsds_below_2"] == round(100 * float((rm[:, :5].min(1) < 2).mean()), 2)
    assert s["centroid_below_5"] == round(100 * float((ce[:, 0] < 5).mean()), 2)
    assert s["steric_clash_fraction"] == round(100 * float((mc < 0.4).mean()), 2)
    assert s["top1_rec_lig_steric_clashes_fraction"] == round(100 * float((cl[:, 0] > 0).mean()), 2)
    assert s["top1_rec_lig_steric_clashes_mean"] == round(float(cl[:, 0].mean()), 2)
    assert "top1_sidechain_rmsds_below_1" not in s          # one of the two complexes is rigid
    s_flex = E.summarize([metrics[0]])
    assert s_flex["top1_sidechain_rmsds_below_1"] == round(100 * float((metrics[0].sc_rmsd[0] < 1).item()), 2)


def test_summarize_top5_uses_the_best_of_the_first_five():
    def pm(r):
        r = torch.tensor(r, dtype=torch.float32)
        z = torch.zeros_like(r)
        return E.PoseMetrics(r, r, z.int(), r, z + 3, z + 1, z.int())
    s = E.summarize([pm([3.0, 4.0, 1.5, 9.0, 9.0, 0.1]), pm([0.5, 9.0, 9.0, 9.0, 9.0, 9.0])])
    assert s["top1_rmsds_below_2"] == 50.0 and s["top5_rmsds_below_2"] == 100.0 and s["top5_centroid_below_2"] == 100.0
    assert s["rmsds_below_2"] == round(100 * 3 / 12, 2) and s["steric_clash_fraction"] == 0.0


# ---------------------------------------------------------------------------------------------- exports
def test_evaluation_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ddp_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(ddp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name in ("ddp_pose_rmsd", "ddp_pose_contacts"):
        assert name in declared and name in L.EXPORTS
    m = re.search(r"#define DDP_EVAL_MAX_ATOMS (\d+)", header)
    assert m and int(m.group(1)) == L.DDP_EVAL_MAX_ATOMS
    import diffdock_pocket_amd as D
    assert D.PoseEvaluator is E.PoseEvaluator and D.summarize is E.summarize
