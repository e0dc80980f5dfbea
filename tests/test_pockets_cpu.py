"""The geometric pocket finder (diffdock_pocket_amd/pockets.py) on the CPU against the tests' own NumPy statement of its definition
(pockets_ref.py): fp32 / fp64 agreement, the 3dpf fixture in seven orientations, synthetic proteins with carved cavities, the driver and
the command line, and the ABI declarations."""
import csv
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pockets_ref as REF
from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import inputs as I
from diffdock_pocket_amd import outputs as O
from diffdock_pocket_amd import pockets as P
from test_inference_csv import Stub, StubConfidence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# Rotation.random(random_state=i).as_matrix(), i = 0 ... 5 (scipy 1.15), and np.random.default_rng(0).uniform(-3, 3, 3) drawn six times in
# that order; applied about the protein's centroid c: x' = R (x - c) + c + t
MOTIONS = [
    ([[0.7582987881957592, -0.3215355579360719, 0.5670959643689784], [0.6267381525729955, 0.1201875342142642, -0.7699053479025089], [0.17939407997543105, 0.939238969380122, 0.2926566631182941]],
     [0.8217701239287258, -1.3812797174167781, -2.7541588563828316]),
    ([[0.7059574172690394, -0.7024198311226546, -0.09072213538298657], [-0.19221011924588954, -0.3132939059336036, 0.9300011820230916], [-0.6816739653693021, -0.6391035200579698, -0.35618435617977917]],
     [-2.9008341868288254, 1.879621435201635, 2.47653346366633]),
    ([[-0.2290941608793594, 0.9494129861783347, 0.21478092821970723], [-0.9367898307621523, -0.2749907030481432, 0.21634446195293677], [0.26446300011835294, -0.15164133642587296, 0.9523991950098314]],
     [0.6398146546030792, 1.3769793659039902, 0.261749948792537]),
    ([[0.9418327109232576, 0.27957662208022427, -0.18651556777159142], [0.17490170924830953, 0.06616203706859464, 0.9823604109251115], [0.2869852552605577, -0.9578410605299533, 0.013415141664819663]],
     [2.610434542726609, 1.8951213247291925, -2.9835689989791114]),
    ([[-0.4394002511939926, 0.8299878262701122, 0.3435805982503526], [-0.7713855759629477, -0.1526356821995688, -0.6177917462347519], [-0.4603169695405198, -0.5364909661521676, 0.7073087945092624]],
     [2.1444256595254156, -2.798486548167214, 1.3779326785796648]),
    ([[-0.9177127151653663, 0.1487453221276309, 0.3683452206408527], [-0.24178594075068924, -0.9448643429742172, -0.22084141874024685], [0.3151871369188713, -0.2917296737067523, 0.9030785492967024]],
     [-1.946066276384646, 2.1790735340993193, 0.24876732149455005]),
]


def fixture_3dpf():
    pdb = open(os.path.join(GOLDEN, "3dpf_protein.pdb")).read()
    sdf = open(os.path.join(GOLDEN, "3dpf_ligand.sdf")).read()
    pos, radii, ca = REF.pdb_heavy_atoms(pdb)
    lig = I.ligand_graph(I.parse_sdf(sdf))[1].astype(np.float64)
    return pdb, pos, radii, ca, lig


def moved(x, motion, c):
    R, t = np.array(motion[0]), np.array(motion[1])
    return (x.astype(np.float64) - c) @ R.T + c + t


def two_cavity_block(r_big=6.5, r_small=5.5):
    """Carbon atoms on a 2 A lattice filling [0, 26]^3 with two spherical cavities carved around lattice points: (8, 8, 8) of radius
    r_big and (18, 18, 18) of radius r_small.  With reach 1.7 + 1.4 = 3.1 A the lattice is watertight and the free space of a cavity
    is the ball of radius about r - 3.1 around its centre, symmetric about it (the grid points have integer coordinates)."""
    ax = np.arange(14) * 2.0
    pts = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    c1, c2 = np.array([8.0, 8.0, 8.0]), np.array([18.0, 18.0, 18.0])
    keep = (np.linalg.norm(pts - c1, axis=1) >= r_big) & (np.linalg.norm(pts - c2, axis=1) >= r_small)
    pos = pts[keep].astype(np.float32)
    return pos, np.full(pos.shape[0], 1.7), pos[::7].copy(), c1, c2


def assert_same_table(pockets, table, rel=0.0):
    assert [(p.label, p.size, p.score) for p in pockets] == [(r["label"], r["size"], r["score"]) for r in table]
    for p, r in zip(pockets, table):
        for got, want in ((p.center, r["center"]), (p.ca_center, r["ca_center"]), (p.points, r["points"])):
            assert got.shape == want.shape and np.abs(got - want).max() <= rel * np.abs(want).max()


def assert_same_grid(grid, ref):
    assert tuple(grid.dims) == tuple(ref["dims"]) and np.array_equal(grid.lo, ref["lo"])
    assert np.array_equal(grid.occ, ref["occ"]) and np.array_equal(grid.bur, ref["bur"]) and np.array_equal(grid.labels, ref["labels"])


# ---------------------------------------------------------------------------------------------- fp32 and fp64
@pytest.fixture(scope="module")
def ref_3dpf():
    pdb, pos, radii, ca, lig = fixture_3dpf()
    table, grid = REF.find_pockets(pos, radii, ca)
    return dict(pdb=pdb, pos=pos, radii=radii, ca=ca, lig=lig, table=table, grid=grid)


def test_the_package_reads_the_same_atoms_as_the_reference(ref_3dpf):
    pos, radii, ca = P.protein_atoms(ref_3dpf["pdb"])
    assert pos.dtype == np.float32 and pos.shape == (1282, 3) and ca.shape == (163, 3)
    assert np.array_equal(pos, ref_3dpf["pos"]) and np.array_equal(radii, ref_3dpf["radii"]) and np.array_equal(ca, ref_3dpf["ca"])


def test_cpu_path_equals_the_fp32_reference_exactly_on_3dpf(ref_3dpf):
    pockets, grid = P.find_pockets(ref_3dpf["pdb"], "cpu", return_grid=True)
    assert_same_grid(grid, ref_3dpf["grid"])
    assert_same_table(pockets, ref_3dpf["table"], rel=1e-12)
    assert len(pockets) == 1                         # default parameters: exactly one pocket survives


@pytest.mark.parametrize("case", ["3dpf", "block"])
def test_fp32_and_fp64_agree_except_at_borderline_points(case, ref_3dpf):
    if case == "3dpf":
        pos, radii, ca, g32 = ref_3dpf["pos"], ref_3dpf["radii"], ref_3dpf["ca"], ref_3dpf["grid"]
    else:
        # (the block's atoms sit on grid points: shifted off them, so that the distances are generic rather than square roots of integers)
        pos, radii, ca, _, _ = two_cavity_block()
        pos = (pos + np.array([0.137, 0.291, 0.413], dtype=np.float32)).astype(np.float32)
        g32 = REF.find_pockets(pos, radii, ca)[1]
    g64 = REF.find_pockets(pos, radii, ca, fp64=True)[1]
    border = g64["border"]
    share = float(border.mean())
    print(f"{case}: borderline share {share:.5%}, fp32 != fp64 at {int((g32['occ'] != g64['occ']).sum())} points")
    assert share <= 0.002                            # the condition of the comparison, not a measurement
    assert not ((g32["occ"] != g64["occ"]) & ~border).any()


# ---------------------------------------------------------------------------------------------- 3dpf in seven orientations
@pytest.mark.parametrize("k", range(7))
def test_3dpf_top_pocket_is_the_ligand_site_in_every_orientation(k, ref_3dpf):
    pos, radii, ca, lig = (ref_3dpf[n] for n in ("pos", "radii", "ca", "lig"))
    if k > 0:
        c = pos.astype(np.float64).mean(0)
        pos, ca, lig = (moved(x, MOTIONS[k - 1], c) for x in (pos, ca, lig))
        pos, ca = pos.astype(np.float32), ca.astype(np.float32)
    pockets = P.find_pockets_atoms(pos, radii, ca, "cpu")
    assert len(pockets) >= 1
    want, _ = I.binding_pocket(ca, lig.astype(np.float32))
    d_center, d_ca = float(np.linalg.norm(pockets[0].center - want)), float(np.linalg.norm(pockets[0].ca_center - want))
    print(f"orientation {k}: center {d_center:.2f} A, ca_center {d_ca:.2f} A from the reference's pocket centre, {len(pockets)} pocket(s)")
    assert d_center <= 5.0 and d_ca <= 5.0
    if k == 0:
        near = np.linalg.norm(lig[:, None, :] - pockets[0].points[None, :, :], axis=-1).min(1) < 3.0
        print(f"ligand heavy atoms within 3 A of a pocket point: {near.mean():.1%}")
        assert near.mean() >= 0.70
        # ranking is invariant under a reordering of the atoms (looser settings, so that there is a ranking: three pockets)
        cfg = P.PocketConfig(min_lines=5)
        base = P.find_pockets_atoms(pos, radii, ca, "cpu", cfg)
        perm = np.random.default_rng(3).permutation(pos.shape[0])
        again = P.find_pockets_atoms(pos[perm], radii[perm], ca[::-1].copy(), "cpu", cfg)
        assert len(base) == 3 and [(p.label, p.size, p.score) for p in base] == [(p.label, p.size, p.score) for p in again]
        for a, b in zip(base, again):
            assert np.array_equal(a.center, b.center) and np.allclose(a.ca_center, b.ca_center, rtol=0, atol=1e-9)


# ---------------------------------------------------------------------------------------------- synthetic proteins
def test_two_carved_cavities_are_found_and_ranked_by_size():
    pos, radii, ca, c1, c2 = two_cavity_block()
    pockets, grid = P.find_pockets_atoms(pos, radii, ca, "cpu", return_grid=True)
    table, ref = REF.find_pockets(pos, radii, ca)
    assert_same_grid(grid, ref)
    assert_same_table(pockets, table, rel=1e-12)
    assert len(pockets) == 2 and pockets[0].size > pockets[1].size and pockets[0].score > pockets[1].score
    assert np.linalg.norm(pockets[0].center - c1) <= 1.0 and np.linalg.norm(pockets[1].center - c2) <= 1.0
    assert pockets[0].score == 7 * pockets[0].size           # a closed cavity: every line is blocked on both sides
    # fewer than min_points points: nothing survives; max_pockets caps the list, best first
    assert P.find_pockets_atoms(pos, radii, ca, "cpu", P.PocketConfig(min_points=pockets[0].size + 1)) == []
    only_big = P.find_pockets_atoms(pos, radii, ca, "cpu", P.PocketConfig(min_points=pockets[1].size + 1))
    assert [p.label for p in only_big] == [pockets[0].label]
    capped = P.find_pockets_atoms(pos, radii, ca, "cpu", P.PocketConfig(max_pockets=1))
    assert [p.label for p in capped] == [pockets[0].label]


def test_a_cavity_too_small_gives_none_and_bad_inputs_raise():
    pos, radii, ca, _, _ = two_cavity_block(r_big=4.1, r_small=0.0)      # one small cavity: the 3 x 3 x 3 points around (8, 8, 8)
    pockets, grid = P.find_pockets_atoms(pos, radii, ca, "cpu", P.PocketConfig(min_points=27), return_grid=True)
    assert int((grid.labels >= 0).sum()) == 27 and [p.size for p in pockets] == [27]
    assert P.find_pockets_atoms(pos, radii, ca, "cpu", P.PocketConfig(min_points=28)) == []       # one point short: none
    with pytest.raises(ValueError):
        P.find_pockets_atoms(np.zeros((0, 3), np.float32), np.zeros(0), ca, "cpu")
    with pytest.raises(ValueError):
        P.find_pockets_atoms(np.array([[0, 0, 0], [3000, 3000, 3000]], np.float32), np.ones(2), ca, "cpu")      # >= 2^31 grid points
    with pytest.raises(ValueError):
        P.find_pockets_atoms(pos, radii, ca, "cpu", P.PocketConfig(spacing=0.0))
    # waters, HETATM records and hydrogens are not part of the protein
    pdb = open(os.path.join(GOLDEN, "3dpf_protein.pdb")).read()
    extra = ("HETATM 9001 ZN    ZN A 900      10.000  25.000  14.000  1.00  0.00          ZN\n"
             "HETATM 9002  O   HOH A 901      11.000  25.000  14.000  1.00  0.00           O\n"
             "ATOM   9003  H   GLY A 902      12.000  25.000  14.000  1.00  0.00           H\n")
    a, b = P.protein_atoms(pdb), P.protein_atoms(pdb.replace("END", extra + "END", 1) if "END" in pdb else pdb + extra)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_config_defaults():
    c = P.PocketConfig()
    assert (c.spacing, c.probe, c.ray_length, c.min_lines, c.min_points, c.margin, c.ca_cutoff, c.max_pockets) == \
        (1.0, 1.4, 10.0, 6, 20, 2.0, 5.0, 16)
    assert {f: getattr(c, f) for f in REF.DEFAULTS} == REF.DEFAULTS


# ---------------------------------------------------------------------------------------------- driver and command line
def test_flags_parse_and_default_to_off():
    p = INF._parser()
    a = p.parse_args([])
    assert a.find_pockets is False and a.pockets_top_k == 1
    assert (a.pocket_spacing, a.pocket_min_lines, a.pocket_probe) == (1.0, 6, 1.4)
    assert INF.pocket_config_from_args(a) is None
    a = p.parse_args(["--find_pockets", "--pockets_top_k", "3", "--pocket_spacing", "0.7", "--pocket_min_lines", "5", "--pocket_probe", "1.2"])
    cfg = INF.pocket_config_from_args(a)
    assert a.find_pockets is True and a.pockets_top_k == 3 and cfg == P.PocketConfig(spacing=0.7, min_lines=5, probe=1.2)


def _rows(tmp_path):
    p = tmp_path / "complexes.csv"
    p.write_text("complex_name,experimental_protein,ligand,pocket_center_x,pocket_center_y,pocket_center_z,flexible_sidechains\n"
                 "given,3dpf_protein.pdb,3dpf_ligand.sdf,8.0,25.0,14.0\n"
                 "found,3dpf_protein.pdb,3dpf_ligand.sdf\n"
                 "missing,no_such_protein.pdb,3dpf_ligand.sdf\n")
    return str(p)


def test_rows_are_expanded_and_an_explicit_centre_wins(tmp_path):
    rows = INF.load_protein_ligand_csv(_rows(tmp_path))
    cfg = P.PocketConfig(min_lines=5)                      # three pockets on 3dpf
    one = INF.expand_pocket_rows(rows, GOLDEN, "cpu", cfg, 1)
    assert [r["complex_name"] for r in one] == ["given", "found", "missing"]
    assert one[0] is rows[0] and one[0]["pocket_center"] == [8.0, 25.0, 14.0] and "pockets" not in one[0]
    found = one[1]["pockets"]
    assert len(found) == 3 and one[1]["pocket_center"] == [float(v) for v in found[0].ca_center] and one[1]["pockets_docked"] == 1
    assert "pocket_error" in one[2] and "pockets" not in one[2]
    two = INF.expand_pocket_rows(rows, GOLDEN, "cpu", cfg, 2)
    assert [r["complex_name"] for r in two] == ["given", "found_pocket1", "found_pocket2", "missing"]
    assert [r["pocket_center"] for r in two[1:3]] == [[float(v) for v in found[k].ca_center] for k in range(2)]
    assert all(r["esm_name"] == "found" and r["pockets_docked"] == 2 and len(r["pockets"]) == 3 for r in two[1:3])
    five = INF.expand_pocket_rows(rows, GOLDEN, "cpu", cfg, 5)            # K above what was found: every pocket once
    assert [r["complex_name"] for r in five] == ["given", "found_pocket1", "found_pocket2", "found_pocket3", "missing"]
    none = INF.expand_pocket_rows(rows, GOLDEN, "cpu", P.PocketConfig(min_points=10 ** 6), 1)
    assert "no pocket found" in none[1]["pocket_error"]


def _run(csv_path, out_dir, **kw):
    return INF.run_csv(csv_path, Stub(), torch.device("cpu"), confidence_model=StubConfidence(), samples_per_complex=3,
                       inference_steps=2, root=GOLDEN, seed=2, allow_zero_esm=True, out_dir=out_dir, **kw)


def test_run_csv_docks_at_the_found_centre_and_writes_pockets_csv(tmp_path):
    path = _rows(tmp_path)
    plain = _run(path, str(tmp_path / "plain"))
    cfg = P.PocketConfig(min_lines=5)
    res = _run(path, str(tmp_path / "pockets"), find_pockets=cfg, pockets_top_k=2)
    assert [r.name for r in plain] == ["given", "found", "missing"]
    assert [r.name for r in res] == ["given", "found_pocket1", "found_pocket2", "missing"]
    # without the option nothing new exists; the row with an explicit centre is the same with it
    assert all(r.pockets is None and not any(f.endswith("pockets.csv") for f in r.files) for r in plain)
    assert res[0].pockets is None and torch.equal(res[0].ligand_pos, plain[0].ligand_pos) and torch.equal(res[0].order, plain[0].order)
    assert sorted(os.path.basename(f) for f in res[0].files) == sorted(os.path.basename(f) for f in plain[0].files)
    assert plain[2].skipped is not None and res[3].skipped is not None and res[3].ligand_pos is None
    want = P.find_pockets(open(os.path.join(GOLDEN, "3dpf_protein.pdb")).read(), "cpu", cfg)
    for k, r in enumerate(res[1:3]):
        assert r.skipped is None and r.ligand_pos.shape[0] == 3 and len(r.pockets) == 3
        # docked at ca_center: the graph's frame is centred there
        assert np.allclose(np.asarray(r.original_center).reshape(3), want[k].ca_center.astype(np.float32), rtol=0, atol=1e-6)
        d = os.path.dirname(r.files[0])
        assert os.path.basename(d) == f"index{k + 1}___found_pocket{k + 1}"
        csvs = [f for f in r.files if os.path.basename(f) == "pockets.csv"]
        assert len(csvs) == 1 and os.path.dirname(csvs[0]) == d
        with open(csvs[0], newline="") as f:
            lines = list(csv.DictReader(f))
        assert list(lines[0].keys()) == O.POCKETS_COLUMNS == ["pocket", "score", "size", "center_x", "center_y", "center_z",
                                                             "ca_center_x", "ca_center_y", "ca_center_z", "docked"]
        assert len(lines) == 3 and [int(x["docked"]) for x in lines] == [1, 1, 0]
        for j, (x, p) in enumerate(zip(lines, want)):
            assert int(x["pocket"]) == j + 1 and int(x["score"]) == p.score and int(x["size"]) == p.size
            assert max(abs(float(x[f"center_{a}"]) - p.center[i]) for i, a in enumerate("xyz")) < 1e-4
            assert max(abs(float(x[f"ca_center_{a}"]) - p.ca_center[i]) for i, a in enumerate("xyz")) < 1e-4
    # a protein on which nothing survives fails the row with a clear message
    bad = _run(path, str(tmp_path / "none"), find_pockets=P.PocketConfig(min_points=10 ** 6))
    assert [r.name for r in bad] == ["given", "found", "missing"] and bad[0].skipped is None
    assert bad[1].skipped is not None and "no pocket found" in bad[1].skipped and bad[1].ligand_pos is None and bad[1].files == []


# ---------------------------------------------------------------------------------------------- ABI
def test_entries_are_declared_exported_and_built():
    header = open(os.path.join(ROOT, "include", "ddp_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(ddp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    names = ("ddp_pocket_occupancy", "ddp_pocket_buriedness", "ddp_pocket_label")
    for name in names:
        assert name in declared and name in L.EXPORTS
    assert set(L.EXPORTS) == declared and len(L.EXPORTS) == len(declared)
    assert "#define DDP_ABI_VERSION 17" in header
    build = __import__("diffdock_pocket_amd.build", fromlist=["SOURCES"])
    assert "ddp_pockets.hip" in build.SOURCES and any(h.endswith("ddp_pockets_uf.h") for h in build.HEADERS)
    assert os.path.exists(L.LIB_PATH), "build the library first (python -m diffdock_pocket_amd.build)"
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in names:
        assert hasattr(lib, name)
    lib.ddp_abi_version.restype = ctypes.c_int
    assert lib.ddp_abi_version() == 17
