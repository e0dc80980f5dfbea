"""The per-residue interaction profile on the host (diffdock_pocket_amd/interactions.py): the PyTorch fp64 form against the independent
NumPy restatement of tests/interactions_ref.py within the derived bound at the shapes the device test uses, the sum over the residues
against PoseScorer, the poison rule, the crystal pose of the 3dpf fixture, both receptor sources, the bit arithmetic on hand-made
vectors, the residue tables, the ABI declarations, and run_csv / the command line with the stub model of test_inference_csv."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import interactions_ref as IR
from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import interactions as IA
from diffdock_pocket_amd import outputs as O
from diffdock_pocket_amd import scoring as SC
from test_evaluation_cpu import graph_3dpf
from test_scoring_cpu import CFG, CSV, _rows, _run, fixture_3dpf, perturbed_poses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


# ---------------------------------------------------------------------------------------------- fixtures
def _sizes_90():
    """90 residues, 1100 atoms: sizes 0 .. 30, an empty residue first, in the middle and last."""
    rng = np.random.default_rng(90)
    sizes = rng.integers(1, 31, 90)
    sizes[[0, 45, 89]] = 0
    free = [r for r in range(90) if r not in (0, 45, 89)]
    while sizes.sum() != 1100:
        r = free[int(rng.integers(0, len(free)))]
        if sizes.sum() > 1100 and sizes[r] > 1:
            sizes[r] -= 1
        elif sizes.sum() < 1100 and sizes[r] < 30:
            sizes[r] += 1
    return sizes


# name: (S, n, residue sizes, keyword arguments of interactions_ref.random_case)
SHAPES = {
    "one_pair": (4, 1, [1], {}),
    "five_single_atom_residues": (4, 3, [1] * 5, {}),                               # R > 4 waves and R % 4 != 0
    "one_past_a_wave": (4, 65, [1, 64, 65], {}),                                   # on both axes; fewer residues than waves
    "ragged_90": (4, 37, _sizes_90(), dict(untyped_residue=7)),                     # m = 1100 > 1024, empty residues, one wholly untyped
    "atom_limit": (2, 1024, [3, 5], {}),
    "ligand_untyped": (4, 5, [2, 3, 1], dict(ligand_untyped=True)),
    "per_sample_receptors": (4, 37, [3, 0, 9, 14, 1, 70, 8], dict(per_sample_rec=True)),
}


def case(name):
    """(x, lig_r, lig_f, rec, rec_r, rec_f, res_ptr as torch tensors, the restatement's result); drawn and referenced once."""
    if name not in _CACHE:
        S, n, sizes, kw = SHAPES[name]
        *arrays, ref = IR.random_case(S, n, sizes, 1000 + sorted(SHAPES).index(name), **kw)
        _CACHE[name] = ([torch.from_numpy(a) for a in arrays], ref)
    return _CACHE[name]


def check_profile(p, b, ref, what="", bits_where=None):
    """profile [S, R, 7] and bits [S, R] (tensors) against the restatement; pairs has to be an exact integer."""
    p, b = p.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(p[..., 6], np.round(p[..., 6]))
    IR.check(p[..., :4], p[..., 4], p[..., 5], p[..., 6].astype(np.int64), b, ref, what, bits_where)


def profile_3dpf():
    """(full-PDB profiler, graph profiler) of the 3dpf fixture; built once."""
    if "prof" not in _CACHE:
        g, pdb, full = fixture_3dpf()
        _CACHE["prof"] = (IA.InteractionProfiler(g, receptor=(full, IA.receptor_residues(pdb))), IA.InteractionProfiler(g))
    return _CACHE["prof"]


# ---------------------------------------------------------------------------------------------- 1. the PyTorch form against the restatement
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_torch_form_matches_the_numpy_restatement(name):
    t, ref = case(name)
    p, b = IA.profile_torch(*t, CFG, 4.5)
    S, n, sizes, kw = SHAPES[name]
    assert p.dtype == torch.float64 and p.shape == (S, len(sizes), 7) and b.dtype == torch.uint8 and b.shape == (S, len(sizes))
    check_profile(p, b, ref, name)
    assert ref["threshold_gap"] >= 1e-6
    if name == "ragged_90":
        assert sum(sizes) == 1100 and len(sizes) == 90 and max(sizes) <= 30 and sizes[0] == sizes[45] == sizes[89] == 0
        assert bool((t[1] < 0).any()) and bool((t[4] < 0).any())                    # untyped atoms on both sides
        for r in (0, 7, 45, 89):                                                     # empty or wholly untyped: the no-pair result
            assert torch.equal(p[:, r, :5], torch.zeros(S, 5, dtype=torch.float64)) and bool(torch.isinf(p[:, r, 5]).all())
            assert not p[:, r, 6].any() and not b[:, r].any()
        assert set(np.unique(ref["bits"]).tolist()) >= {0, 1, 3, 5, 7} and (ref["terms"].sum((0, 1)) > 0).all()   # every term and bit
    if name == "ligand_untyped":
        assert not ref["pairs"].any() and not b.any() and bool(torch.isinf(p[..., 5]).all())
    if name == "per_sample_receptors":
        assert t[3].dim() == 3 and not torch.equal(p[0], p[1])


def test_sum_over_the_residues_is_the_scorers_inter():
    g, pdb, full = fixture_3dpf()
    x = perturbed_poses()
    full_pf, graph_pf = profile_3dpf()
    for pf, receptor in ((full_pf, full), (graph_pf, "graph")):
        out = pf.profile(x)
        sc = SC.PoseScorer(g, receptor=receptor).score(x)
        t = pf._cpu
        ref = IR.profile(x.numpy(), t["lig_r"].numpy(), t["lig_f"].numpy(), t["rec"].numpy(), t["rec_r"].numpy(), t["rec_f"].numpy(), t["ptr"].numpy())
        bt, be = IR.bounds(ref)
        err_t = (out.terms.sum(1) - sc.terms).abs().numpy()
        err_e = (out.energy.sum(1) - sc.inter).abs().numpy()
        print("sum over residues: worst |err| / summed bound", float((err_t / bt.sum(1)).max()), float((err_e / be.sum(1)).max()))
        assert (err_t <= bt.sum(1)).all() and (err_e <= be.sum(1)).all()
        assert int(out.pairs.sum()) == int(ref["pairs"].sum()) > 0


# ---------------------------------------------------------------------------------------------- 2. the poison rule
def poison_cases():
    """(tensors with the poison, the clean tensors, the entries [S, R] that have to be poisoned) for: a NaN and an inf in one typed
    ligand atom of sample 1; a NaN and an inf in one typed receptor atom of one residue of sample 2 (per-sample receptors); the same
    values in untyped atoms, which poison nothing."""
    t, ref = case("per_sample_receptors")
    x, lig_r, lig_f, rec, rec_r, rec_f, ptr = t
    S, R = rec.shape[0], ptr.shape[0] - 1
    i = int(torch.nonzero(lig_r >= 0)[2])
    res = 5
    j = int(ptr[res]) + int(torch.nonzero(rec_r[int(ptr[res]):int(ptr[res + 1])] >= 0)[3])
    ui, uj = int(torch.nonzero(lig_r < 0)[0]), int(torch.nonzero(rec_r < 0)[0])
    out = []
    for bad in (float("nan"), float("inf"), float("-inf")):
        xb = x.clone()
        xb[1, i, 2] = bad
        want = torch.zeros(S, R, dtype=torch.bool)
        want[1] = True
        out.append(([xb] + t[1:], t, want))
        rb = rec.clone()
        rb[2, j, 0] = bad
        want = torch.zeros(S, R, dtype=torch.bool)
        want[2, res] = True
        out.append((t[:3] + [rb] + t[4:], t, want))
        xb, rb = x.clone(), rec.clone()
        xb[0, ui, 1] = bad
        rb[3, uj, 1] = bad
        out.append(([xb] + t[1:3] + [rb] + t[4:], t, torch.zeros(S, R, dtype=torch.bool)))
    return out


def check_poison(run):
    """run(tensors) -> (profile [S, R, 7], bits [S, R]): the poisoned entries are NaN / 0 / 0, every other entry keeps its bits."""
    clean = None
    for bad_t, clean_t, want in poison_cases():
        if clean is None:
            clean = [a.cpu() for a in run(clean_t)]
        p, b = (a.cpu() for a in run(bad_t))
        assert bool(torch.isnan(p[..., :6][want]).all()) and not p[..., 6][want].any() and not b[want].any()
        keep = ~want
        assert torch.equal(p[keep].view(torch.int64), clean[0][keep].view(torch.int64)) and torch.equal(b[keep], clean[1][keep])
        assert not bool(torch.isnan(p[keep]).any())


def test_poison_rule():
    check_poison(lambda t: IA.profile_torch(*t, CFG, 4.5))
    # the restatement states the same rule
    for bad_t, _, want in poison_cases():
        ref = IR.profile(*[a.numpy() for a in bad_t])
        assert np.array_equal(np.isnan(ref["energy"]), want.numpy())


# ---------------------------------------------------------------------------------------------- 3. the crystal pose of 3dpf
def test_crystal_pose_of_3dpf():
    g, pdb, full = fixture_3dpf()
    pf, _ = profile_3dpf()
    assert pf.n_res == 163 and len(pf.labels) == 163 and pf._cpu["rec"].shape == (1282, 3) and int(pf._cpu["ptr"][-1]) == 1282
    out = pf.profile(g["ligand"].pos.float()[None])
    assert out.terms.shape == (1, 163, 4) and out.terms.dtype == torch.float64 and out.pairs.dtype == torch.int64 and out.bits.dtype == torch.uint8
    b = out.bits[0]
    assert [int(((b & k) != 0).sum()) for k in (IA.CONTACT, IA.HYDROPHOBIC_BIT, IA.HBOND_BIT)] == [23, 17, 7]
    hbond = [pf.labels[r] for r in torch.nonzero(b & IA.HBOND_BIT).flatten().tolist()]
    assert hbond == ["A:LEU160", "A:ALA161", "A:LEU214", "A:PRO217", "A:ALA220", "A:ARG222", "A:SER228"]
    best = int(out.energy[0].argmin())
    print("most favourable residue", pf.labels[best], float(out.energy[0, best]))
    assert pf.labels[best] == "A:TYR219" and abs(float(out.energy[0, best]) - -1.859) < 1e-3
    sc = SC.PoseScorer(g, receptor=full).score(g["ligand"].pos.float()[None])
    t = pf._cpu
    ref = IR.profile(g["ligand"].pos.float()[None].numpy(), t["lig_r"].numpy(), t["lig_f"].numpy(), t["rec"].numpy(), t["rec_r"].numpy(),
                     t["rec_f"].numpy(), t["ptr"].numpy())
    assert abs(float(out.energy.sum()) - float(sc.inter)) <= float(IR.bounds(ref)[1].sum())
    check_profile(torch.cat([out.terms, out.energy[..., None], out.d_min[..., None], out.pairs.double()[..., None]], -1), out.bits, ref, "3dpf")
    import diffdock_pocket_amd as DP
    assert DP.InteractionProfiler is IA.InteractionProfiler and DP.ProfileConfig is IA.ProfileConfig


def test_both_receptor_sources_give_identical_rows():
    g, pdb, full = fixture_3dpf()
    full_pf, graph_pf = profile_3dpf()
    x = perturbed_poses()
    a, b = full_pf.profile(x), graph_pf.profile(x)
    tab = IA.receptor_residues(pdb)
    atom_res = tab.index()
    pos = g["atom"].pos.float().numpy()
    first = graph_pf.table.ptr[:-1]
    assert graph_pf.n_res == g["receptor"].x.shape[0] and (np.diff(graph_pf.table.ptr) > 0).all()
    rows = [int(atom_res[int(np.abs(full.coords - pos[int(j)]).sum(1).argmin())]) for j in first]
    assert len(set(rows)) == len(rows)
    for r_graph, r_full in enumerate(rows):
        assert graph_pf.labels[r_graph] == f"{r_graph}:{full_pf.labels[r_full].split(':')[1][:3]}"
    rows = torch.tensor(rows)
    assert torch.equal(a.terms[:, rows], b.terms) and torch.equal(a.energy[:, rows], b.energy) and torch.equal(a.d_min[:, rows], b.d_min)
    assert torch.equal(a.pairs[:, rows], b.pairs) and torch.equal(a.bits[:, rows], b.bits) and int(b.pairs.sum()) > 0
    # flexible graph: each sample's own atoms
    gf, _ = graph_3dpf(flex="A:160-A:193-A:197")
    pf = IA.InteractionProfiler(gf)
    apos = gf["atom"].pos.float()[None].repeat(4, 1, 1).contiguous()
    e0 = pf.profile(x[:4], atom_pos=apos)
    assert torch.equal(e0.energy, pf.profile(x[:4]).energy)
    j = int(torch.cdist(x[2].double(), apos[2].double()).min(0).values.argmin())
    r = int(torch.as_tensor(gf["atom", "receptor"].edge_index)[1][j])
    apos[2, j] += 30.0
    e1 = pf.profile(x[:4], atom_pos=apos)
    changed = (e1.energy != e0.energy)
    assert bool(changed[2, r]) and int(changed.sum()) == 1
    with pytest.raises(ValueError):
        pf.profile(x[:4], atom_pos=apos[:2])
    with pytest.raises(ValueError):
        pf.profile(x[:, :5])
    with pytest.raises(ValueError):
        IA.InteractionProfiler(gf, receptor="pdb")
    with pytest.raises(ValueError):
        IA.InteractionProfiler(gf, config=IA.ProfileConfig(contact_distance=0.0))
    assert pf.profile(x[:0]).bits.shape == (0, pf.n_res)


# ---------------------------------------------------------------------------------------------- 4. the bits
def test_tanimoto_recovery_and_frequency_on_hand_made_bits():
    C, Hy, Hb = IA.CONTACT, IA.HYDROPHOBIC_BIT, IA.HBOND_BIT
    bits = torch.tensor([[C | Hy, C, 0, Hb],          # 4 bits set
                         [C, C | Hb, 0, 0],           # 3 bits set, 2 shared with row 0
                         [0, 0, 0, 0],
                         [0, 0, 0, 0]], dtype=torch.uint8)
    R = bits.shape[1]
    prof = IA.InteractionProfile(torch.zeros(4, R, 4, dtype=torch.float64), torch.zeros(4, R, dtype=torch.float64),
                                 torch.zeros(4, R, dtype=torch.float64), torch.zeros(4, R, dtype=torch.int64), bits, list("abcd"))
    sim = prof.similarity()
    assert sim.shape == (4, 4) and sim.dtype == torch.float64 and torch.equal(sim, sim.T)
    assert sim[0, 0] == 1.0 and sim[0, 1] == 2.0 / 5.0 and sim[0, 2] == 0.0 and sim[2, 3] == 1.0 and sim[2, 2] == 1.0   # both empty: 1
    assert prof.tanimoto_to(bits[1]).tolist() == [0.4, 1.0, 0.0, 0.0] and prof.tanimoto_to(bits[2]).tolist() == [0.0, 0.0, 1.0, 1.0]
    assert prof.recovery(bits[0]).tolist() == [1.0, 0.5, 0.0, 0.0] and prof.recovery(bits[1]).tolist()[:2] == [2.0 / 3.0, 1.0]
    assert bool(torch.isnan(prof.recovery(bits[2])).all())                            # an empty reference
    f = prof.frequency()
    assert f.shape == (R, 3) and f.tolist() == [[0.5, 0.25, 0.0], [0.5, 0.0, 0.25], [0.0, 0.0, 0.0], [0.0, 0.0, 0.25]]
    assert torch.equal(IA.tanimoto(bits, bits), sim) and torch.equal(IA.recovery(bits, bits[0]), prof.recovery(bits[0]))
    sub = prof.index(torch.tensor([1, 0]))
    assert torch.equal(sub.bits, bits[[1, 0]]) and sub.labels == prof.labels and prof.cpu().bits.device.type == "cpu"


# ---------------------------------------------------------------------------------------------- 5. residue tables
def test_residue_tables_and_the_non_monotone_index():
    g, pdb, full = fixture_3dpf()
    tab = IA.receptor_residues(pdb)
    assert len(tab.labels) == 163 and tab.ptr.dtype == np.int32 and int(tab.ptr[-1]) == len(full.radii) == 2463 and tab.ptr[0] == 0
    assert tab.labels[0].startswith("A:") and re.fullmatch(r"A:[A-Z]{3}\d+", tab.labels[0])
    assert np.array_equal(np.bincount(tab.index(), minlength=163), np.diff(tab.ptr))
    kept = tab.keep(full.radii >= 0)
    assert kept.labels == tab.labels and int(kept.ptr[-1]) == 1282
    gt = IA.graph_residues(g)
    index = torch.as_tensor(g["atom", "receptor"].edge_index)[1].numpy()
    assert len(gt.labels) == g["receptor"].x.shape[0] and np.array_equal(gt.index(), index) and gt.labels[0] == "0:MET"
    t = IA.ResidueTable.from_index([0, 0, 2, 2, 2], ["a", "b", "c"])               # residue b is empty
    assert t.ptr.tolist() == [0, 2, 2, 5]
    with pytest.raises(ValueError, match="non-decreasing"):
        IA.ResidueTable.from_index([0, 1, 0], ["a", "b"])
    with pytest.raises(ValueError):
        IA.ResidueTable(np.array([0, 3, 2, 5], dtype=np.int32), ["a", "b", "c"]).check()
    with pytest.raises(ValueError):
        IA.InteractionProfiler(g, receptor=(full, IA.ResidueTable(tab.ptr[:-1], tab.labels[:-1])))      # does not end at m
    import copy
    bad = copy.deepcopy(g)
    ei = torch.as_tensor(bad["atom", "receptor"].edge_index).clone()
    ei[1, 0], ei[1, -1] = ei[1, -1].clone(), ei[1, 0].clone()
    bad["atom", "receptor"].edge_index = ei
    with pytest.raises(ValueError, match="non-decreasing"):
        IA.InteractionProfiler(bad)


# ---------------------------------------------------------------------------------------------- 6. ABI
def test_entry_is_declared_exported_and_built():
    header = open(os.path.join(ROOT, "include", "ddp_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(ddp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert "ddp_pose_profile" in declared and "ddp_pose_profile" in L.EXPORTS and set(L.EXPORTS) == declared
    assert "#define DDP_ABI_VERSION 17" in header and "ddp_profile_args_t" in header
    assert "ddp_profile.hip" in __import__("diffdock_pocket_amd.build", fromlist=["SOURCES"]).SOURCES
    assert os.path.exists(L.LIB_PATH), "build the library first (python -m diffdock_pocket_amd.build)"
    lib = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(lib, "ddp_pose_profile")
    lib.ddp_abi_version.restype = ctypes.c_int
    assert lib.ddp_abi_version() == 17
    # the ctypes mirror has the size the header's struct has on this ABI: 6 int32, 7 pointers, 12 doubles, 2 pointers
    assert ctypes.sizeof(L.ProfileArgs) == 24 + 7 * 8 + 12 * 8 + 2 * 8
    # the host-side checks of the entry need no device: they return before any launch
    lib.ddp_pose_profile.argtypes, lib.ddp_pose_profile.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    assert lib.ddp_pose_profile(None, None) == -1
    assert lib.ddp_pose_profile(ctypes.byref(L.ProfileArgs(n_samples=0, n_res=3)), None) == 0
    assert lib.ddp_pose_profile(ctypes.byref(L.ProfileArgs(n_samples=2, n_res=0)), None) == 0
    assert lib.ddp_pose_profile(ctypes.byref(L.ProfileArgs(n_samples=1, n=L.DDP_EVAL_MAX_ATOMS + 1, m=0, n_res=1)), None) == -2
    assert lib.ddp_pose_profile(ctypes.byref(L.ProfileArgs(n_samples=1, n=4, m=0, n_res=1)), None) == -1          # null pointers
    assert lib.ddp_pose_profile(ctypes.byref(L.ProfileArgs(n_samples=1, n=4, m=0, n_res=-1)), None) == -1


# ---------------------------------------------------------------------------------------------- 7. driver and command line
def test_flags_parse_and_default_to_off():
    p = INF._parser()
    a = p.parse_args([])
    assert a.interaction_profile is False and a.interaction_contact_distance == 4.5
    a = p.parse_args(["--interaction_profile", "--interaction_contact_distance", "4.0"])
    assert a.interaction_profile is True and a.interaction_contact_distance == 4.0
    import inspect
    assert inspect.signature(INF.run_csv).parameters["interaction_profile"].default is None


def test_run_csv_writes_the_profile_and_leaves_everything_else_alone(tmp_path):
    p = tmp_path / "complexes.csv"
    p.write_text(CSV)
    plain = _run(str(p), str(tmp_path / "plain"), evaluate=True)
    prof = _run(str(p), str(tmp_path / "prof"), evaluate=True, interaction_profile=IA.ProfileConfig())
    assert len(prof) == 2
    added = {"interactions.csv", "interaction_summary.csv", "interaction_similarity.csv"}
    assert O.INTERACTIONS_COLUMNS == ["rank", "sample", "residue", "gauss", "repulsion", "hydrophobic", "hbond", "energy", "d_min", "contact",
                                      "hydrophobic_bit", "hbond_bit"]
    assert O.INTERACTION_SUMMARY_COLUMNS == ["residue", "contact_freq", "hydrophobic_freq", "hbond_freq", "mean_energy"]
    for a, b in zip(plain, prof):
        assert a.skipped is None and b.skipped is None and a.interactions is None and a.interaction_reference is None
        assert torch.equal(a.ligand_pos, b.ligand_pos) and torch.equal(a.confidence, b.confidence) and torch.equal(a.order, b.order)
        old = {os.path.basename(f): f for f in a.files}
        new = {os.path.basename(f): f for f in b.files}
        assert set(new) - set(old) == added and set(old) <= set(new) and not added & set(os.listdir(os.path.dirname(a.files[0])))
        assert set(os.listdir(os.path.dirname(b.files[0]))) == set(new) and set(os.listdir(os.path.dirname(a.files[0]))) == set(old)
        for name, path in old.items():
            assert open(path, "rb").read() == open(new[name], "rb").read(), name
        it = b.interactions
        assert isinstance(it, IA.InteractionProfile) and not it.bits.is_cuda and it.bits.shape[0] == 4 and it.terms.shape[2] == 4
        assert b.interaction_reference.bits.shape == (1, it.bits.shape[1])
        rows = _rows(new["interactions.csv"])
        assert list(rows[0].keys()) == O.INTERACTIONS_COLUMNS and len(rows) == int((it.pairs > 0).sum()) > 0
        k = 0
        for s in range(4):
            for r in torch.nonzero(it.pairs[s] > 0).flatten().tolist():
                row = rows[k]
                k += 1
                assert int(row["rank"]) == s + 1 and int(row["sample"]) == int(b.order[s]) and row["residue"] == it.labels[r]
                for col, val in (("gauss", it.terms[s, r, 0]), ("repulsion", it.terms[s, r, 1]), ("hydrophobic", it.terms[s, r, 2]),
                                 ("hbond", it.terms[s, r, 3]), ("energy", it.energy[s, r])):
                    assert abs(float(row[col]) - float(val)) <= 1e-5 * abs(float(val)) + 1e-12, col
                assert abs(float(row["d_min"]) - float(it.d_min[s, r])) < 1e-4
                assert [int(row["contact"]), int(row["hydrophobic_bit"]), int(row["hbond_bit"])] == [(int(it.bits[s, r]) >> j) & 1 for j in range(3)]
        rows = _rows(new["interaction_summary.csv"])
        reached = torch.nonzero((it.pairs > 0).any(0)).flatten().tolist()
        assert list(rows[0].keys()) == O.INTERACTION_SUMMARY_COLUMNS and [r["residue"] for r in rows] == [it.labels[r] for r in reached]
        f = it.frequency()
        for row, r in zip(rows, reached):
            assert abs(float(row["contact_freq"]) - float(f[r, 0])) < 1e-4 and abs(float(row["hbond_freq"]) - float(f[r, 2])) < 1e-4
            assert abs(float(row["mean_energy"]) - float(it.energy[:, r].mean())) <= 1e-5 * abs(float(it.energy[:, r].mean())) + 1e-12
        rows = _rows(new["interaction_similarity.csv"])
        assert list(rows[0].keys()) == ["rank", "sample", "tanimoto_to_rank1", "tanimoto_to_reference", "recovery_of_reference"]
        assert len(rows) == 4 and float(rows[0]["tanimoto_to_rank1"]) == 1.0 and [int(r["sample"]) for r in rows] == b.order.tolist()
        rb = b.interaction_reference.bits[0]
        for s, row in enumerate(rows):
            assert abs(float(row["tanimoto_to_rank1"]) - float(it.tanimoto_to(it.bits[0])[s])) < 1e-4
            assert abs(float(row["tanimoto_to_reference"]) - float(it.tanimoto_to(rb)[s])) < 1e-4
            assert abs(float(row["recovery_of_reference"]) - float(it.recovery(rb)[s])) < 1e-4
    # the two rows took the two receptor forms: the rigid row against the full PDB with its labels, the flexible row against its own
    # atom nodes with the graph's; the reference is the crystal pose through the same profiler
    g, pdb, full = fixture_3dpf()
    full_pf, _ = profile_3dpf()
    want = full_pf.profile(prof[1].ligand_pos)
    assert torch.equal(want.energy, prof[1].interactions.energy) and torch.equal(want.bits, prof[1].interactions.bits)
    assert prof[1].interactions.labels == full_pf.labels and prof[0].interactions.labels[0] == "0:MET"
    assert torch.equal(prof[1].interaction_reference.bits, full_pf.profile(g["ligand"].pos.float()[None]).bits)
    assert int(((prof[1].interaction_reference.bits[0] & IA.HBOND_BIT) != 0).sum()) == 7
    # without evaluate the similarity file has three columns
    path = O.write_interaction_similarity_csv(str(tmp_path / "sim.csv"), prof[1].interactions, prof[1].order)
    assert list(_rows(path)[0].keys()) == O.INTERACTION_SIMILARITY_COLUMNS == ["rank", "sample", "tanimoto_to_rank1"]
