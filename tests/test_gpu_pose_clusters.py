"""ddp_pose_pairwise_rmsd and ddp_pose_cluster on the device: the all-pairs matrix bit for bit against ddp_pose_rmsd with ref = pose i
(every tile width, ragged last tiles, the edges of the 256-lane stride over the permutations), the row-selection path, the guards,
reproducibility, the greedy rule against its numpy statement, and PoseEvaluator.cluster on the poses of a short device Sampler run."""
import numpy as np
import pytest
import torch

from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import evaluation as E
from diffdock_pocket_amd import launch as LA
from test_pose_clusters_cpu import np_greedy, np_pairwise

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _table(n, P, seed):
    """Synthetic atom-major permutation table [n, P]: column 0 the identity, the others random permutations of 0 .. n-1."""
    gen = torch.Generator().manual_seed(seed)
    cols = [torch.arange(n)] + [torch.randperm(n, generator=gen) for _ in range(P - 1)]
    return torch.stack(cols, 1).to(torch.int32).contiguous()


def _poses(S, rows, seed):
    return (torch.randn(S, rows, 3, generator=torch.Generator().manual_seed(seed)) * 3).contiguous()


def _check_bitwise(pos, perms_t, sel=None):
    """dist[i, j] (i < j) = pose_rmsd of pose j against ref = the selected rows of pose i, bit for bit; mirror and diagonal."""
    S = pos.shape[0]
    dist = LA.pose_pairwise_rmsd(pos, perms_t, sel)
    assert dist.shape == (S, S) and dist.dtype == torch.float32
    for i in range(S - 1):
        ref = (pos[i] if sel is None else pos[i][sel.long()]).contiguous()
        want, _ = LA.pose_rmsd(pos[i + 1:], ref, perms_t, sel=sel)
        assert torch.equal(_bits(dist[i, i + 1:]), _bits(want)), (S, perms_t.shape, i)
    assert torch.equal(_bits(dist), _bits(dist.T)) and (_bits(dist.diagonal()) == 0).all()
    return dist


@pytest.mark.parametrize("S", [1, 2, 3, 5, 41])
def test_pairwise_equals_pose_rmsd_bit_for_bit(S):
    dev = _dev()
    for n in (1, 7, 33):
        pos = _poses(S, n, seed=S * 100 + n).to(dev)
        for P in (1, 12, 255, 256, 257, 1000):
            _check_bitwise(pos, _table(n, P, seed=P).to(dev))


@pytest.mark.parametrize("n", [33, 300, 600])
def test_pairwise_ragged_tiles_at_every_tile_width(n):
    """S = T + 1 (one full tile in row 0), 2 T (the second tile of row 0 is ragged) and 2 T + 1, for T = 8 / 4 / 2."""
    dev = _dev()
    T = LA.pairwise_tile(n)
    assert T == {33: 8, 300: 4, 600: 2}[n]
    perms_t = _table(n, 3, seed=n).to(dev)
    for S in (T + 1, 2 * T, 2 * T + 1):
        _check_bitwise(_poses(S, n, seed=S).to(dev), perms_t)


def test_pairwise_at_the_atom_limit():
    dev = _dev()
    n = L.DDP_EVAL_MAX_ATOMS
    _check_bitwise(_poses(3, n, seed=1).to(dev), _table(n, 2, seed=2).to(dev))
    x = torch.zeros(2, n + 1, 3, device=dev)
    with pytest.raises(L.DdpError, match="DDP_EVAL_MAX_ATOMS"):
        LA.pose_pairwise_rmsd(x, torch.arange(n + 1, dtype=torch.int32, device=dev)[:, None].contiguous())
    empty = LA.pose_pairwise_rmsd(x[:0], torch.arange(5, dtype=torch.int32, device=dev)[:, None].contiguous())
    assert empty.shape == (0, 0) and empty.is_cuda
    torch.cuda.synchronize()


def test_pairwise_row_selection_against_the_torch_form():
    """Side-chain style: 11 selected rows of 50 (pos_stride = 150 > 3 n), identity permutation."""
    dev = _dev()
    pos = _poses(7, 50, seed=4)
    sel = torch.tensor([49, 3, 17, 0, 22, 8, 41, 30, 5, 12, 48], dtype=torch.int32)
    ident = torch.arange(11, dtype=torch.int32)[:, None].contiguous()
    dist = _check_bitwise(pos.to(dev), ident.to(dev), sel.to(dev))
    want = E._pairwise_torch(pos, ident.T, sel=sel.long())
    assert torch.allclose(dist.cpu().double(), want.double(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(dist.cpu().double().numpy(), np_pairwise(pos[:, sel.long()].numpy(), ident.T.numpy()), rtol=1e-5, atol=1e-6)


def test_pairwise_guards():
    dev = _dev()
    n, S = 7, 5
    pos = _poses(S, n, seed=9).to(dev)
    good = _table(n, 4, seed=3)
    # one column with an entry outside [0, n): the result of the other columns
    for bad_entry in (n, -1):
        t = good.clone()
        t[4, 2] = bad_entry
        got = LA.pose_pairwise_rmsd(pos, t.to(dev))
        want = LA.pose_pairwise_rmsd(pos, good[:, [0, 1, 3]].contiguous().to(dev))
        assert torch.equal(_bits(got), _bits(want))
    # no valid column: NaN off the diagonal, the diagonal stays 0
    t = good.clone()
    t[0, :] = n
    got = LA.pose_pairwise_rmsd(pos, t.to(dev)).cpu()
    off = ~torch.eye(S, dtype=torch.bool)
    assert got[off].isnan().all() and (got.diagonal() == 0).all()
    # a selected row outside the sample's stride: never read; stride and sel are shared, so it is a row of every sample and
    # every pair is NaN
    for bad_row in (n, -2):
        sel = torch.arange(n, dtype=torch.int32)
        sel[3] = bad_row
        got = LA.pose_pairwise_rmsd(pos, good.to(dev), sel=sel.to(dev)).cpu()
        assert got[off].isnan().all() and (got.diagonal() == 0).all()
    torch.cuda.synchronize()


def test_pairwise_is_bitwise_reproducible():
    dev = _dev()
    pos, t = _poses(41, 33, seed=6).to(dev), _table(33, 1000, seed=7).to(dev)
    a, b = LA.pose_pairwise_rmsd(pos, t), LA.pose_pairwise_rmsd(pos, t)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(a.T)) and (_bits(a.diagonal()) == 0).all()
    out = torch.full((41, 41), -1.0, device=dev)
    assert LA.pose_pairwise_rmsd(pos, t, out=out) is out and torch.equal(_bits(out), _bits(a))


def _synthetic_matrix(S, cutoff, seed):
    """Distances of random points in the plane (several poses per cluster), some entries exactly at the cutoff, one NaN pose."""
    gen = torch.Generator().manual_seed(seed)
    pts = torch.randn(S, 2, generator=gen) * (1.0 + S ** 0.5 / 2)
    d = torch.cdist(pts, pts).float()
    d = torch.triu(d, 1) + torch.triu(d, 1).T
    for _ in range(max(1, S // 4)):
        a, b = torch.randint(0, S, (2,), generator=gen).tolist()
        if a != b:
            d[a, b] = d[b, a] = cutoff
    if S > 2:
        k = int(torch.randint(0, S, (1,), generator=gen))
        d[k, :] = d[:, k] = float("nan")
        d[k, k] = 0.0
    return d.contiguous()


@pytest.mark.parametrize("S", [1, 2, 7, 64, 65, 257, 1024])
def test_cluster_equals_the_numpy_greedy_rule(S):
    dev = _dev()
    cutoff = 2.0
    d = _synthetic_matrix(S, cutoff, seed=S)
    gen = torch.Generator().manual_seed(S + 1)
    shuffled = torch.randperm(S, generator=gen).to(torch.int32)
    holed = shuffled.clone()
    holed[S // 2] = S + 3                               # one entry that is no pose: the pose it replaced is never named
    for order in (None, shuffled, holed):
        labels, reps, sizes, count = LA.pose_cluster(d.to(dev), None if order is None else order.to(dev), cutoff)
        want = np_greedy(d.numpy(), None if order is None else order.tolist(), cutoff)
        assert labels.cpu().tolist() == want[0].tolist() and reps.cpu().tolist() == want[1].tolist()
        assert sizes.cpu().tolist() == want[2].tolist() and int(count) == want[3]
    assert labels.dtype == torch.int32 and (S > 1 or labels.cpu().tolist() == [-1])      # S = 1: the only pose was never named


def test_cluster_limits():
    dev = _dev()
    with pytest.raises(L.DdpError, match="1024"):
        LA.pose_cluster(torch.zeros(1025, 1025, device=dev))
    labels, reps, sizes, count = LA.pose_cluster(torch.zeros(0, 0, device=dev))
    assert labels.shape == (0,) and int(count) == 0
    torch.cuda.synchronize()


def test_device_sampler_poses_cluster_like_the_torch_form():
    from diffdock_pocket_amd.diffusion import get_t_schedule
    from diffdock_pocket_amd.sampler import Sampler, SamplerConfig
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    from oracle.cases import CASES
    from helpers import case_inputs
    from test_gpu_parity import _model_for
    dev = _dev()
    case = CASES["cfg2_noflex"]
    _, _, _, sd = case_inputs(case.name)
    model = _model_for(case, sd)
    g = make_3dpf_complex(seed=0, flexible_sidechains=False, n_rec=16)
    smp = Sampler(model, g, 6, dev, SamplerConfig(inference_steps=4, flexible_sidechains=False), seed=3)
    smp.randomize()
    sched = get_t_schedule(4)
    for i in range(4):
        smp.step(i, sched)
    lig = smp.lig_pos.clone()
    smp.close()
    ev, ev_cpu = E.PoseEvaluator(g, dev), E.PoseEvaluator(g)
    exact = np_pairwise(lig.cpu().numpy(), ev_cpu._cpu["perms"].numpy())
    v = np.sort(exact[np.triu_indices(6, 1)])
    k = int(np.argmax(np.diff(v)))
    cutoff = float((v[k] + v[k + 1]) / 2)                # the midpoint of the largest gap: neither form can sit on it
    conf = torch.tensor([0.3, -0.2, 0.9, 0.1, 0.5, -1.0])
    for c in (None, conf):
        got = ev.cluster(lig, None if c is None else c.to(dev), cutoff)
        assert got.dist.is_cuda and got.labels.is_cuda
        got = got.cpu()
        want = ev_cpu.cluster(lig.cpu(), c, cutoff)
        assert torch.allclose(got.dist.double(), want.dist.double(), rtol=1e-5, atol=1e-6)
        assert torch.equal(got.labels, want.labels) and torch.equal(got.representatives, want.representatives)
        assert torch.equal(got.sizes, want.sizes) and got.by_size() == want.by_size()
        assert torch.allclose(got.rmsd_to_representative.double(), want.rmsd_to_representative.double(), rtol=1e-5, atol=1e-6)
