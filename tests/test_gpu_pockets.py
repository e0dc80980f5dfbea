"""The pocket finder's kernels (csrc/ddp_pockets.hip) against the tests' NumPy statement of the definition (pockets_ref.py): exact
occupancy, buriedness and label arrays at the smallest shapes where each kernel can go wrong, the whole pipeline on the device against
the reference's table and against the CPU path, and the argument guards."""
import ctypes as C

import numpy as np
import pytest
import torch

import pockets_ref as REF
from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import launch as K
from diffdock_pocket_amd import pockets as P
from test_pockets_cpu import MOTIONS, fixture_3dpf, moved, two_cavity_block

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRIDS = [(1, 1, 70), (5, 7, 9), (64, 64, 3), (33, 65, 17)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------- occupancy
def _atoms(dims, n, spacing, lo, seed):
    """n atoms around a grid: inside, on its faces, and outside it (some reaching in, some not), radii of several sizes."""
    rng = np.random.default_rng(seed)
    lo = np.asarray(lo, dtype=np.float64)
    hi = lo + (np.array(dims) - 1) * spacing
    pos = rng.uniform(lo - 5.0, hi + 5.0, size=(n, 3))
    inside = rng.random(n) < 0.6
    pos[inside] = rng.uniform(lo, hi, size=(int(inside.sum()), 3)) if inside.any() else pos[inside]
    for a in range(0, n, 5):            # on a face: one coordinate exactly on the first or the last grid plane
        ax = a % 3
        pos[a, ax] = (lo if (a // 3) % 2 == 0 else hi)[ax]
    radii = rng.choice([0.3, 0.45, 0.8, 1.2, 2.3] if n > 100 else [0.45, 1.2, 3.1, 4.7, 7.3], size=n)      # (many atoms: small ones, or all is full)
    return pos.astype(np.float32), (radii ** 2).astype(np.float32)


@pytest.mark.parametrize("n_atoms", [1, 2, 300])
@pytest.mark.parametrize("dims", GRIDS)
def test_occupancy_is_exact(dims, n_atoms):
    for spacing, lo in ((1.0, (-3.0, 2.0, 11.0)), (0.7, (-3.55, 2.125, 10.7))):
        pos, r2 = _atoms(dims, n_atoms, spacing, lo, seed=n_atoms + dims[0])
        lo32 = np.asarray(lo, dtype=np.float32)
        want = REF.occupancy(pos, r2, lo32, spacing, dims)
        got = K.pocket_occupancy(dev(pos), dev(r2), lo32, np.float32(spacing), dims)
        again = K.pocket_occupancy(dev(pos), dev(r2), lo32, np.float32(spacing), dims, occ=torch.full(dims, 7, dtype=torch.uint8, device=DEV))
        assert got.shape == tuple(dims) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), want) and torch.equal(got, again)
        if n_atoms == 300:
            assert want.any()


@pytest.mark.parametrize("dims", GRIDS)
def test_occupancy_of_spheres_that_cover_the_grid_or_miss_it(dims):
    lo, s = np.array([1.5, -2.0, 0.25], dtype=np.float32), 1.0
    mid = lo + (np.array(dims) - 1) * s / 2
    diag = float(np.linalg.norm((np.array(dims) - 1) * s))
    # one atom in the middle whose sphere covers everything; one far outside that covers everything; one outside that reaches nothing
    for pos, r, full in (([mid], [diag], True), ([mid + 500.0], [1000.0 + diag], True), ([lo - 30.0], [5.0], False),
                         ([mid + np.array([0, 0, 1e6], dtype=np.float32)], [5.0], False)):
        pos, r2 = np.asarray(pos, dtype=np.float32), (np.asarray(r, dtype=np.float64) ** 2).astype(np.float32)
        want = REF.occupancy(pos, r2, lo, s, dims)
        got = K.pocket_occupancy(dev(pos), dev(r2), lo, np.float32(s), dims).cpu().numpy()
        assert np.array_equal(got, want) and bool(want.all()) == full and bool(want.any()) == full


# ---------------------------------------------------------------------------------------------- buriedness
def _shell():
    occ = np.zeros((12, 12, 12), dtype=np.uint8)
    occ[3:9, 3:9, 3:9] = 1
    occ[4:8, 4:8, 4:8] = 0
    return occ


def _tube():
    occ = np.zeros((12, 12, 12), dtype=np.uint8)
    occ[4:8, 4:8, :] = 1
    occ[5:7, 5:7, :] = 0           # a 2 x 2 channel along z, open at both ends of the grid
    return occ


def _random_occ(dims, fill, seed):
    return (np.random.default_rng(seed).random(dims) < fill).astype(np.uint8)


OCC_CASES = {
    "shell": _shell(), "tube": _tube(), "empty": np.zeros((5, 7, 9), np.uint8), "full": np.ones((5, 7, 9), np.uint8),
    "thin z": _random_occ((64, 64, 3), 0.3, 1), "line": _random_occ((1, 1, 70), 0.2, 2),
    "random 5%": _random_occ((33, 65, 17), 0.05, 3), "random 30%": _random_occ((33, 65, 17), 0.30, 4),
    "random 60%": _random_occ((5, 7, 9), 0.60, 5), "random 20% small": _random_occ((5, 7, 9), 0.20, 6),
}


@pytest.mark.parametrize("name", list(OCC_CASES))
def test_buriedness_is_exact(name):
    occ = OCC_CASES[name]
    for spacing in (0.7, 1.0):
        for ray in (3.0, 10.0):
            steps = REF.ray_steps(spacing, ray)
            assert steps == {(0.7, 3.0): (4, 2), (0.7, 10.0): (14, 8), (1.0, 3.0): (3, 1), (1.0, 10.0): (10, 5)}[(spacing, ray)]
            want = REF.buriedness(occ, spacing, ray)
            for min_lines in (0, 4, 6):
                bur, mask = K.pocket_buriedness(dev(occ), spacing, ray, min_lines)
                assert np.array_equal(bur.cpu().numpy(), want), (name, spacing, ray)
                want_mask = np.where(REF.pocket_mask(occ, want, min_lines), want.astype(np.int32) + 1, 0)
                assert mask.dtype == torch.int32 and np.array_equal(mask.cpu().numpy(), want_mask)
            if name == "shell" and ray == 10.0:
                assert (want[4:8, 4:8, 4:8] == 7).all() and (want[occ == 0].reshape(-1).sum() == 7 * 64)     # inside 7, outside 0
            if name == "tube" and ray == 10.0:
                assert (want[5:7, 5:7, 3:9] == 6).all()            # the z line is missing
            if name in ("empty", "full"):
                assert not want.any()


# ---------------------------------------------------------------------------------------------- labelling
def _serpentine():
    """A one-voxel-wide path through 32 x 32 x 4: full rows at even i, joined at alternating ends through the odd rows, in the layers
    k = 0 and k = 2, and one voxel in layer 1 that joins the two layers at the far end: a single chain of some 1100 voxels."""
    m = np.zeros((32, 32, 4), dtype=np.int32)
    for k in (0, 2):
        m[0::2, :, k] = 1
        for i in range(1, 32, 2):
            m[i, 31 if (i // 2) % 2 == 0 else 0, k] = 1
    m[30, 31, 1] = 1
    return m


def _edge_and_corner():
    m = np.zeros((6, 6, 6), dtype=np.int32)
    m[0:2, 0:2, 0:2] = 1
    m[2:4, 2:4, 0:2] = 1          # touches the first across an edge only
    m[4:6, 4:6, 2:4] = 1          # touches the second across a corner only
    return m


def _tree():
    """One component that reaches every 256-point tile of a 16 x 16 x 16 grid (a tile is one i-slab) and crosses every tile boundary."""
    m = np.zeros((16, 16, 16), dtype=np.int32)
    m[:, 0, 0] = 1
    m[:, :, 0] = 1
    ii, jj = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    m[(ii + jj) % 2 == 0, :] = 1
    return m


def _random_mask(dims, fill, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(dims) < fill, rng.integers(1, 9, size=dims), 0).astype(np.int32)      # non-zero = in the mask


def _checkerboard():
    i, j, k = np.meshgrid(np.arange(7), np.arange(9), np.arange(11), indexing="ij")
    return ((i + j + k) % 2).astype(np.int32)


MASK_CASES = {
    "serpentine": _serpentine(), "edge and corner": _edge_and_corner(), "tree": _tree(), "checkerboard": _checkerboard(),
    "empty": np.zeros((5, 7, 9), np.int32), "full": np.ones((33, 65, 17), np.int32), "full line": np.ones((1, 1, 70), np.int32),
    **{f"random {int(100 * f)}% {d}": _random_mask(d, f, s) for s, (f, d) in enumerate(
        [(f, d) for f in (0.10, 0.31, 0.60) for d in ((5, 7, 9), (33, 65, 17))])},
}


@pytest.mark.parametrize("name", list(MASK_CASES))
def test_labels_are_exact_and_reproducible(name):
    mask = MASK_CASES[name]
    want = REF.label(mask)
    got = K.pocket_label(dev(mask))
    again = K.pocket_label(dev(mask), labels=torch.full(mask.shape, 123, dtype=torch.int32, device=DEV))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, again)
    flat = want.reshape(-1)
    if name in ("serpentine", "tree", "full", "full line"):
        assert set(np.unique(flat).tolist()) - {-1} == {int(np.nonzero(mask.reshape(-1))[0][0])}            # one component
    if name == "serpentine":
        assert int((mask != 0).sum()) > 1000
    if name == "edge and corner":
        assert len(set(np.unique(flat).tolist()) - {-1}) == 3                                              # they stay apart
    if name == "checkerboard":
        inside = flat >= 0
        assert np.array_equal(flat[inside], np.nonzero(inside)[0])                                         # every point its own


# ---------------------------------------------------------------------------------------------- the whole pipeline
def _pipeline_inputs(case):
    if case == "block":
        pos, radii, ca, _, _ = two_cavity_block()
        return pos, radii, ca
    _, pos, radii, ca, _ = fixture_3dpf()
    if case == "3dpf rotated":
        c = pos.astype(np.float64).mean(0)
        pos, ca = (moved(x, MOTIONS[2], c).astype(np.float32) for x in (pos, ca))
    return pos, radii, ca


@pytest.mark.parametrize("case", ["3dpf", "3dpf rotated", "block"])
def test_device_pipeline_equals_the_reference_and_the_cpu_path(case):
    pos, radii, ca = _pipeline_inputs(case)
    table, ref = REF.find_pockets(pos, radii, ca)
    pockets, grid = P.find_pockets_atoms(pos, radii, ca, DEV, return_grid=True)
    cpu, cpu_grid = P.find_pockets_atoms(pos, radii, ca, "cpu", return_grid=True)
    assert len(table) == (2 if case == "block" else 1)
    assert tuple(grid.dims) == tuple(ref["dims"]) and np.array_equal(grid.lo, ref["lo"])
    for name in ("occ", "bur", "labels"):
        assert np.array_equal(getattr(grid, name), ref[name]), name
        assert np.array_equal(getattr(grid, name), getattr(cpu_grid, name)), name
    assert [(p.label, p.size, p.score) for p in pockets] == [(r["label"], r["size"], r["score"]) for r in table]
    assert [(p.label, p.size, p.score) for p in pockets] == [(p.label, p.size, p.score) for p in cpu]
    for p, r, q in zip(pockets, table, cpu):
        for got, want, other in ((p.center, r["center"], q.center), (p.ca_center, r["ca_center"], q.ca_center), (p.points, r["points"], q.points)):
            assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
            assert np.array_equal(got, other)             # the two paths of pockets.py share the host part: the same bits


def test_find_pockets_on_the_device_from_pdb_text_and_looser_settings():
    pdb = fixture_3dpf()[0]
    cfg = P.PocketConfig(min_lines=5, spacing=0.7)
    a, b = P.find_pockets(pdb, DEV, cfg), P.find_pockets(pdb, "cpu", cfg)
    assert len(a) >= 2 and [(p.label, p.size, p.score) for p in a] == [(p.label, p.size, p.score) for p in b]
    assert all(np.array_equal(x.ca_center, y.ca_center) and np.array_equal(x.center, y.center) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- guards
def test_guards_return_einval_and_write_nothing():
    lib = L.load()
    pos, r2 = dev(np.zeros((2, 3), np.float32)), dev(np.ones(2, np.float32))
    occ = torch.full((4, 4, 4), 9, dtype=torch.uint8, device=DEV)
    bur = torch.full((4, 4, 4), 9, dtype=torch.uint8, device=DEV)
    mask = torch.full((4, 4, 4), 9, dtype=torch.int32, device=DEV)
    labels = torch.full((4, 4, 4), 9, dtype=torch.int32, device=DEV)
    st, p = K.stream(), lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)

    def occupancy(pos_=p(pos), r2_=p(r2), n=2, s=1.0, dims=(4, 4, 4), occ_=p(occ)):
        return lib.ddp_pocket_occupancy(pos_, r2_, n, 0.0, 0.0, 0.0, s, dims[0], dims[1], dims[2], occ_, st)

    def buriedness(occ_=p(occ), dims=(4, 4, 4), s=1.0, ray=10.0, min_lines=6, bur_=p(bur), mask_=p(mask)):
        return lib.ddp_pocket_buriedness(occ_, dims[0], dims[1], dims[2], s, ray, min_lines, bur_, mask_, st)

    def label(mask_=p(mask), dims=(4, 4, 4), labels_=p(labels)):
        return lib.ddp_pocket_label(mask_, dims[0], dims[1], dims[2], labels_, st)

    bad = [occupancy(pos_=null), occupancy(r2_=null), occupancy(occ_=null), occupancy(n=0), occupancy(n=-3), occupancy(s=0.0),
           occupancy(s=-1.0), occupancy(s=float("nan")), occupancy(dims=(0, 4, 4)), occupancy(dims=(4, -1, 4)), occupancy(dims=(4, 4, 0)),
           occupancy(dims=(2048, 2048, 512)),
           buriedness(occ_=null), buriedness(bur_=null), buriedness(mask_=null), buriedness(dims=(4, 0, 4)), buriedness(s=0.0),
           buriedness(s=-0.5), buriedness(ray=-1.0), buriedness(min_lines=8), buriedness(min_lines=-1), buriedness(dims=(2048, 2048, 512)),
           label(mask_=null), label(labels_=null), label(dims=(4, 4, 0)), label(dims=(-4, 4, 4)), label(dims=(2048, 2048, 512))]
    assert bad == [-1] * len(bad)                        # DDP_EINVAL
    assert b"ddp_pocket_label" in lib.ddp_last_error()
    torch.cuda.synchronize()
    for t in (occ, bur, mask, labels):
        assert bool((t == 9).all())                      # nothing was launched
    # the wrappers turn the same conditions into errors
    with pytest.raises(L.DdpError):
        K.pocket_occupancy(dev(np.zeros((0, 3), np.float32)), dev(np.zeros(0, np.float32)), (0, 0, 0), 1.0, (4, 4, 4))
    with pytest.raises(L.DdpError):
        K.pocket_occupancy(pos, r2, (0, 0, 0), 0.0, (4, 4, 4))
    with pytest.raises(L.DdpError):
        K.pocket_buriedness(torch.zeros((4, 4, 4), dtype=torch.uint8, device=DEV), -1.0, 10.0, 6)
    # and the valid call right after works
    assert occupancy() == 0 and buriedness() == 0 and label() == 0
    torch.cuda.synchronize()
    assert not bool((occ == 9).any()) and not bool((labels == 9).any())
