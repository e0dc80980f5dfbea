"""The argument checks that the pose tools share (PoseScorer, PoseRefiner, InteractionProfiler, PoseEvaluator; the minimisers and the
searcher check through their scorer): one body, so that the tools cannot drift apart in what they accept or in what they say."""
from __future__ import annotations


def check_poses(n: int, n_a: int, device, lig_pos, atom_pos, who: str):
    """ValueError unless lig_pos is [S, n, 3] and atom_pos (if any) [S, n_a, 3] with the same S, device poses live on the `device`
    the tool `who` was built for, and both tensors share a device.  device None: the shapes alone (no device is tested)."""
    if lig_pos.dim() != 3 or lig_pos.shape[1:] != (n, 3):
        raise ValueError(f"lig_pos: expected [S, {n}, 3], got {tuple(lig_pos.shape)}")
    if atom_pos is not None and (atom_pos.dim() != 3 or atom_pos.shape[1:] != (n_a, 3) or atom_pos.shape[0] != lig_pos.shape[0]):
        raise ValueError(f"atom_pos: expected [S, {n_a}, 3], got {tuple(atom_pos.shape)}")
    if device is None:
        return
    if lig_pos.is_cuda and (device.type != "cuda" or lig_pos.device != device):
        raise ValueError(f"poses on {lig_pos.device}, {who} built for {device}")
    if atom_pos is not None and atom_pos.device != lig_pos.device:
        raise ValueError("lig_pos and atom_pos on different devices")


def check_anchor(x, anchor):
    """ValueError unless `anchor` (the start poses of a restraint) has the shape and the device of the poses x."""
    if anchor.shape != x.shape or anchor.device != x.device:
        raise ValueError("anchor: the shape and device of lig_pos")
