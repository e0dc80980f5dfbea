"""Binding modes of sampled poses on the host: the PyTorch form of the all-pairs symmetry-corrected RMSD against a float64 numpy
restatement, the greedy leader rule on hand-written matrices, the ABI declarations, the command-line flag and run_csv / modes.csv
with the stub model of test_inference_csv."""
import csv
import os
import re

import numpy as np
import torch

from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import evaluation as E
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import outputs as O
from test_evaluation_cpu import _edges, benzene, graph_3dpf, perturbed
from test_inference_csv import Stub, StubConfidence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def para_xylene():
    """Ring + two para methyl groups: the two mirror planes through / across the substituents give 4 automorphisms."""
    return [6] * 8, _edges([(i, (i + 1) % 6) for i in range(6)] + [(0, 6), (3, 7)])


def np_pairwise(pos, perms):
    """float64 definition: d[i, j] = min_p sqrt(mean_a |pos_j[a] - pos_i[perms[p, a]]|^2) for i < j, mirrored, zero diagonal."""
    pos = np.asarray(pos, dtype=np.float64)
    S = pos.shape[0]
    d = np.zeros((S, S))
    for i in range(S):
        for j in range(i + 1, S):
            v = np.sqrt(((pos[j][None] - pos[i][perms]) ** 2).sum(-1).mean(-1))
            d[i, j] = d[j, i] = v.min()
    return d


def np_greedy(dist, order, cutoff):
    """The rule of the issue, written out: (labels, reps, sizes, count)."""
    S = dist.shape[0]
    cut = np.float32(cutoff)
    labels, reps, sizes, count = np.full(S, -1), np.full(S, -1), np.full(S, -1), 0
    for o in (range(S) if order is None else order):
        if o < 0 or o >= S or labels[o] >= 0:
            continue
        members = (labels < 0) & ((dist[o] < cut) | (np.arange(S) == o))
        labels[members] = count
        reps[count], sizes[count] = o, int(members.sum())
        count += 1
    return labels, reps, sizes, count


def _poses(n, S, seed):
    ref = torch.randn(n, 3, generator=torch.Generator().manual_seed(seed)) * 2
    return ref, perturbed(ref, S, scale=1.0, seed=seed + 1)


def test_pairwise_torch_matches_the_float64_definition():
    for mol, count in ((benzene, 12), (para_xylene, 4)):
        z, ei = mol()
        perms, ok = E.ligand_automorphisms(z, ei)
        assert ok and perms.shape[0] == count
        ref, pos = _poses(len(z), 6, seed=count)
        pos[4] = pos[1][torch.from_numpy(perms[count - 1]).long()]      # pose 4 = pose 1 relabelled by an automorphism
        got = E._pairwise_torch(pos, torch.from_numpy(perms))
        assert got.dtype == torch.float32 and got.shape == (6, 6)
        np.testing.assert_allclose(got.double().numpy(), np_pairwise(pos.numpy(), perms), rtol=1e-5, atol=1e-6)
        assert float(got[1, 4]) == 0.0 and float(got[4, 1]) == 0.0
        assert torch.equal(got, got.T) and (got.diagonal() == 0).all()
        # without the symmetry the relabelled pose is far away
        plain = E._pairwise_torch(pos, torch.arange(len(z))[None])
        assert float(plain[1, 4]) > 0.1 and (plain + 1e-6 >= got).all()


def test_pairwise_torch_sel_rows_and_small_sample_counts():
    ref, pos = _poses(9, 4, seed=3)
    sel = torch.tensor([7, 2, 5])
    ident = torch.arange(3)[None]
    got = E._pairwise_torch(pos, ident, sel=sel)
    np.testing.assert_allclose(got.double().numpy(), np_pairwise(pos[:, sel].numpy(), ident.numpy()), rtol=1e-5, atol=1e-6)
    assert E._pairwise_torch(pos[:1], ident, sel=sel).tolist() == [[0.0]]
    assert E._pairwise_torch(pos[:0], ident, sel=sel).shape == (0, 0)


def test_evaluator_pairwise_and_cluster_on_3dpf():
    g, _ = graph_3dpf()
    ev = E.PoseEvaluator(g)
    ref = g["ligand"].pos.float()
    lig = (ref[None] + 0.05 * torch.randn((7,) + tuple(ref.shape), generator=torch.Generator().manual_seed(1))).contiguous()
    lig[3:] += 6.0                                   # two groups, far apart
    lig[5] = lig[0][ev._cpu["perms"][-1].long()]     # pose 5 = pose 0 relabelled
    d = ev.pairwise_rmsd(lig)
    np.testing.assert_allclose(d.double().numpy(), np_pairwise(lig.numpy(), ev._cpu["perms"].numpy()), rtol=1e-5, atol=1e-6)
    assert float(d[0, 5]) == 0.0
    c = ev.cluster(lig, cutoff=2.0)
    assert isinstance(c, E.PoseClusters) and c.symmetry_corrected and c.n_modes == 2
    assert c.labels.tolist() == [0, 0, 0, 1, 1, 0, 1] and c.representatives.tolist() == [0, 3] + [-1] * 5
    assert c.sizes.tolist() == [4, 3] + [-1] * 5 and c.by_size() == [0, 1]
    assert torch.equal(c.rmsd_to_representative, torch.stack([d[0, 0], d[0, 1], d[0, 2], d[3, 3], d[3, 4], d[0, 5], d[3, 6]]))
    # by confidence: pose 6 ranks first and leads mode 0; a [S, k] head is ranked by its first column
    conf = torch.tensor([0.1, 0.2, 0.3, 0.0, -1.0, 0.5, 0.9])
    c2 = ev.cluster(lig, confidence=conf)
    assert c2.labels.tolist() == [1, 1, 1, 0, 0, 1, 0] and c2.representatives.tolist()[:2] == [6, 5]
    c3 = ev.cluster(lig, confidence=torch.stack([conf, -conf], 1))
    assert torch.equal(c3.labels, c2.labels) and torch.equal(c3.cpu().dist, c2.dist)
    assert E.PoseEvaluator(g, max_automorphisms=1).cluster(lig).symmetry_corrected is False
    import diffdock_pocket_amd as D
    assert D.PoseClusters is E.PoseClusters


def test_greedy_rule_on_hand_written_matrices():
    nan = float("nan")
    d = torch.tensor([[0.0, 1.0, 2.0, 5.0, nan],
                      [1.0, 0.0, 1.5, 5.0, nan],
                      [2.0, 1.5, 0.0, 1.0, nan],
                      [5.0, 5.0, 1.0, 0.0, nan],
                      [nan, nan, nan, nan, 0.0]])
    # sample order: 0 takes 1; 2 sits exactly at the cutoff and stays out, then leads 3; the NaN pose is alone
    labels, reps, sizes, count = E._cluster_torch(d, None, 2.0)
    assert labels.tolist() == [0, 0, 1, 1, 2] and reps.tolist() == [0, 2, 4, -1, -1] and sizes.tolist() == [2, 2, 1, -1, -1]
    assert count == 3
    # ranked order 3, 4, 1, ...: mode 0 holds rank 1 (pose 3) and pose 2; the NaN pose opens mode 1 and takes nobody
    labels, reps, sizes, count = E._cluster_torch(d, [3, 4, 1, 0, 2], 2.0)
    assert labels.tolist() == [2, 2, 0, 0, 1] and reps.tolist()[:3] == [3, 4, 1] and sizes.tolist()[:3] == [2, 1, 2] and count == 3
    # an entry outside [0, S) is skipped, a pose never named keeps -1
    labels, reps, sizes, count = E._cluster_torch(d, [9, 3, -1], 0.5)
    assert labels.tolist() == [-1, -1, -1, 0, -1] and reps.tolist()[:2] == [3, -1] and sizes.tolist()[:2] == [1, -1] and count == 1
    for order in (None, [3, 4, 1, 0, 2], [4, 4, 0, 7, 2]):
        for cutoff in (0.5, 1.0, 2.0, 6.0):
            got = E._cluster_torch(d, order, cutoff)
            want = np_greedy(d.numpy(), order, cutoff)
            for a, b in zip(got[:3], want[:3]):
                assert a.tolist() == b.tolist()
            assert got[3] == want[3]


def test_by_size_ties_go_to_the_lower_index():
    z = torch.zeros(7)
    c = E.PoseClusters(torch.zeros(7, 7), z.int(), torch.tensor([0, 1, 4, 6, -1, -1, -1], dtype=torch.int32),
                       torch.tensor([2, 3, 1, 3, -1, -1, -1], dtype=torch.int32), z)
    assert c.n_modes == 4 and c.by_size() == [1, 3, 0, 2]


def test_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ddp_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(ddp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name in ("ddp_pose_pairwise_rmsd", "ddp_pose_cluster"):
        assert name in declared and name in L.EXPORTS
    assert "#define DDP_ABI_VERSION 17" in header
    m = re.search(r"#define DDP_PAIRWISE_MAX_SAMPLES (\d+)", header)
    assert m and int(m.group(1)) == L.DDP_PAIRWISE_MAX_SAMPLES


def test_cluster_rmsd_flag_parses_and_defaults_to_off():
    p = INF._parser()
    assert p.parse_args([]).cluster_rmsd is None
    assert p.parse_args(["--cluster_rmsd", "1.5"]).cluster_rmsd == 1.5


def _write_csv(tmp_path):
    p = tmp_path / "complexes.csv"
    p.write_text("complex_name,experimental_protein,ligand,pocket_center_x,pocket_center_y,pocket_center_z,flexible_sidechains\n"
                 "3dpf_rigid,3dpf_protein.pdb,3dpf_ligand.sdf\n")
    return str(p)


def _run(csv_path, out_dir, **kw):
    return INF.run_csv(csv_path, Stub(), torch.device("cpu"), confidence_model=StubConfidence(), samples_per_complex=5,
                       inference_steps=3, root=GOLDEN, seed=2, allow_zero_esm=True, out_dir=out_dir, **kw)


def test_run_csv_attaches_clusters_and_writes_modes_csv(tmp_path):
    csv_path = _write_csv(tmp_path)
    plain = _run(csv_path, str(tmp_path / "plain"))[0]
    assert plain.skipped is None and plain.clusters is None
    names = {os.path.basename(p) for p in plain.files}
    assert names == {"rank1.sdf"} | {f"rank{k + 1}_confidence{float(plain.confidence[k]):.2f}.sdf" for k in range(5)}
    assert set(os.listdir(os.path.dirname(plain.files[0]))) == names

    res = _run(csv_path, str(tmp_path / "modes"), cluster_rmsd=2.0)[0]
    assert res.skipped is None and torch.equal(res.ligand_pos, plain.ligand_pos)
    c = res.clusters
    assert isinstance(c, E.PoseClusters) and c.dist.shape == (5, 5) and not c.dist.is_cuda
    want = E.PoseEvaluator(graph_3dpf()[0]).cluster(res.ligand_pos, cutoff=2.0)
    assert torch.equal(c.dist, want.dist) and torch.equal(c.labels, want.labels) and int(c.labels[0]) == 0
    assert {os.path.basename(p) for p in res.files} == names | {"modes.csv"}
    path = os.path.join(os.path.dirname(res.files[0]), "modes.csv")
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0].keys()) == O.MODES_COLUMNS and len(rows) == 5
    for k, r in enumerate(rows):
        m = int(c.labels[k])
        assert int(r["rank"]) == k + 1 and int(r["sample"]) == int(res.order[k]) and int(r["mode"]) == m
        assert r["confidence"] == f"{float(res.confidence[k]):.4f}"
        assert int(r["is_representative"]) == int(int(c.representatives[m]) == k) and int(r["mode_size"]) == int(c.sizes[m])
        assert abs(float(r["rmsd_to_representative"]) - float(c.rmsd_to_representative[k])) < 1e-4
    assert sum(int(r["is_representative"]) for r in rows) == c.n_modes

    # a tight cutoff: every pose its own mode; no confidence model: the confidence column is empty
    tight = INF.run_csv(csv_path, Stub(), torch.device("cpu"), samples_per_complex=5, inference_steps=3, root=GOLDEN, seed=2,
                        allow_zero_esm=True, out_dir=str(tmp_path / "tight"), cluster_rmsd=1e-6)[0]
    assert tight.clusters.labels.tolist() == [0, 1, 2, 3, 4] and tight.clusters.by_size() == [0, 1, 2, 3, 4]
    with open(os.path.join(os.path.dirname(tight.files[0]), "modes.csv"), newline="") as f:
        assert all(r["confidence"] == "" and r["is_representative"] == "1" for r in csv.DictReader(f))
