"""What the four pose entries (ddp_pose_score, ddp_pose_profile, ddp_pose_minimize, ddp_pose_minimize_flex) share, without a device:
the layout of ddp_score_form_t inside their argument structs and of the ctypes mirrors, the return codes of the host checks the
entries have in common, the argument checker of launch.py, and the definition at a non-default form: the PyTorch forms against the
NumPy restatements at constants that all differ from the defaults (tests/pose_form_cases.py)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import flexmin_ref as F
import interactions_ref as I
import pose_form_cases as P
import vinardo_ref as V
from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import interactions as IA
from diffdock_pocket_amd import launch as LA
from diffdock_pocket_amd import minimize_flex as MF
from diffdock_pocket_amd import scoring as SC

MIRRORS = [(L.ScoreArgs, 72, 184), (L.ProfileArgs, 80, 192), (L.MinimizeArgs, 104, 272), (L.MinimizeFlexArgs, 104, 352)]
NAMES = [k for k, _ in L.ScoreForm._fields_]


# ---------------------------------------------------------------------------------------------- 1. layout
def test_score_form_lists_the_eleven_constants_in_the_header_s_order():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ddp_hip.h")).read()
    body = header[header.rindex("typedef struct {", 0, header.index("} ddp_score_form_t;")):header.index("} ddp_score_form_t;")]
    assert [w.strip() for line in body.splitlines()[1:] for w in line.replace("double", "").strip(" ;").split(",") if w.strip()] == NAMES
    assert NAMES == list(P.FORM) and len(NAMES) == 11 and ctypes.sizeof(L.ScoreForm) == 88
    assert all(t is ctypes.c_double for _, t in L.ScoreForm._fields_)
    for k in NAMES:      # once in the header's structs: the four entries embed the form
        assert len([line for line in header.splitlines() if line.startswith("  double") and k in line.replace(",", " ").replace(";", " ").split()]) == 1, k


@pytest.mark.parametrize("cls,offset,size", MIRRORS, ids=lambda v: getattr(v, "__name__", str(v)))
def test_mirrors_embed_the_form_where_the_flat_fields_were(cls, offset, size):
    assert ctypes.sizeof(cls) == size and cls.form.offset == offset and cls.cutoff.offset == cls.form.offset
    for i, k in enumerate(NAMES):
        assert getattr(cls, k).offset == offset + 8 * i and getattr(cls, k).size == 8, k
    after = [f for f, _ in cls._fields_][[f for f, _ in cls._fields_].index("form") + 1]
    assert getattr(cls, after).offset == offset + 88
    a = cls(**{k: float(i + 1) for i, k in enumerate(NAMES)})                       # flat names in the constructor
    assert [getattr(a.form, k) for k in NAMES] == [float(i + 1) for i in range(11)]
    setattr(a, "hbond_bad", 0.25)                                                    # flat write, read through .form
    assert a.form.hbond_bad == 0.25
    a.form.gauss_offset = -3.5                                                       # and the reverse
    assert a.gauss_offset == -3.5
    a.form = L.ScoreForm.from_config(SC.ScoreConfig(**P.FORM))
    assert {k: getattr(a, k) for k in NAMES} == P.FORM


def test_score_form_from_a_config_carries_each_value_under_its_own_name():
    defaults = SC.ScoreConfig()
    vals = list(P.FORM.values())
    assert len(set(vals)) == 11 and not set(vals) & {getattr(defaults, k) for k in NAMES}
    f = L.ScoreForm.from_config(SC.ScoreConfig(**P.FORM))
    assert {k: getattr(f, k) for k in NAMES} == P.FORM
    g = L.ScoreForm.from_config(SC.ScoreConfig(**P.SWAPPED))
    assert (g.gauss_offset, g.hydrophobic_good, g.hbond_bad) == (P.FORM["hydrophobic_good"], P.FORM["hbond_bad"], P.FORM["gauss_offset"])
    assert {k: getattr(L.ScoreForm.from_config(defaults), k) for k in NAMES} == {k: getattr(defaults, k) for k in NAMES}


# ---------------------------------------------------------------------------------------------- 2. the host checks the entries share
ENTRIES = [("ddp_pose_score", L.ScoreArgs, ("pos", "lig_radii", "lig_flags", "energy"), dict(tor_divisor=1.0), L.DDP_EVAL_MAX_ATOMS),
           ("ddp_pose_profile", L.ProfileArgs, ("pos", "lig_radii", "lig_flags", "res_ptr", "profile", "bits"),
            dict(n_res=1, contact_distance=4.5), L.DDP_EVAL_MAX_ATOMS),
           ("ddp_pose_minimize", L.MinimizeArgs, ("pos", "anchor", "lig_radii", "lig_flags", "step", "accepted", "energy_in", "energy_out"),
            dict(grow=2.0, shrink=0.5, step_max=1024.0), L.DDP_MINIMIZE_MAX_ATOMS),
           ("ddp_pose_minimize_flex", L.MinimizeFlexArgs, ("pos", "anchor", "lig_radii", "lig_flags", "step", "accepted", "energy_in", "energy_out"),
            dict(grow=2.0, shrink=0.5, step_max=1024.0), L.DDP_MINIMIZE_MAX_ATOMS)]
BAD_FORMS = [("cutoff", dict(cutoff=0.0)), ("cutoff", dict(cutoff=-1.0)), ("cutoff", dict(cutoff=math.inf)), ("cutoff", dict(cutoff=math.nan)),
             ("good < bad", dict(gauss_width=0.0)), ("good < bad", dict(hydrophobic_bad=P.FORM["hydrophobic_good"])),
             ("good < bad", dict(hbond_bad=P.FORM["hbond_good"] - 0.1))]


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e[0])
def test_host_checks_return_before_any_launch(entry):
    """Host buffers stand in for the device pointers: every call here returns from the checks in front of the launch, which look at
    no pointer's target.  m = 0: no receptor pointers are asked for."""
    name, cls, pointers, scalars, limit = entry
    assert os.path.exists(L.LIB_PATH), "build the library first (python -m diffdock_pocket_amd.build)"
    lib = ctypes.CDLL(L.LIB_PATH)
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    lib.ddp_last_error.restype = ctypes.c_char_p
    buf = ctypes.create_string_buffer(64)

    def call(**kw):
        a = cls(n_samples=1, n=4, m=0, **scalars)
        a.form = L.ScoreForm.from_config(SC.ScoreConfig(**P.FORM))
        for k in pointers:
            setattr(a, k, ctypes.addressof(buf))
        for k, v in kw.items():
            setattr(a, k, v)
        return fn(ctypes.byref(a), None)

    for text, bad in BAD_FORMS:
        assert call(**bad) == -1, bad
        msg = lib.ddp_last_error().decode()
        assert msg.startswith(name + ":") and text in msg, (bad, msg)
    assert fn(None, None) == -1 and lib.ddp_last_error().decode().startswith(name + ":")
    assert call(n_samples=0) == 0
    assert call(n=limit + 1) == -2
    msg = lib.ddp_last_error().decode()
    assert msg.startswith(name + ":") and ("DDP_EVAL_MAX_ATOMS" if limit == L.DDP_EVAL_MAX_ATOMS else "DDP_MINIMIZE_MAX_ATOMS") in msg
    for bad in (dict(n_samples=-1), dict(n=0), dict(m=-1)):
        assert call(**bad) == -1 and lib.ddp_last_error().decode().startswith(name + ":"), bad
    # the order: shape, then the limit, then the pointers, then the constants
    assert call(n=limit + 1, m=-1) == -1 and call(n=limit + 1, pos=None) == -2
    assert call(pos=None, cutoff=0.0) == -1 and "null" in lib.ddp_last_error().decode()


# ---------------------------------------------------------------------------------------------- 3. the argument checker of launch.py
def test_check_tensors_names_the_tensor_it_rejects():
    dev = torch.device("cpu")
    good = torch.zeros(2, 5, 3)
    rows = lambda t, dt=torch.float32, shape=(2, 5, 3): [(good, torch.float32, (2, 5, 3), "pos"), (t, dt, shape, "anchor")]
    LA.check_tensors("entry", dev, rows(good))
    LA.check_tensors("entry", dev, rows(good, shape=None))
    for what, bad in (("dtype", good.double()), ("shape", torch.zeros(2, 4, 3)), ("strides", torch.zeros(2, 3, 5).transpose(1, 2)),
                      ("device", torch.zeros(2, 5, 3, device="meta")), ("missing", None)):
        with pytest.raises(L.DdpError, match="entry anchor"):
            LA.check_tensors("entry", dev, rows(bad))
    LA.check_tensors("entry", dev, rows(None), optional=("anchor",))
    LA.check_tensors("entry", dev, rows(None), optional=None)
    with pytest.raises(L.DdpError, match="entry anchor: missing"):
        LA.check_tensors("entry", dev, rows(None), optional=("pos",))
    with pytest.raises(ValueError, match="anchor") as e:
        LA.check_tensors("entry", dev, rows(good.double()), error=ValueError)
    assert not isinstance(e.value, L.DdpError)


def test_pose_dims_knows_the_two_receptor_forms():
    pos = torch.zeros(2, 5, 3)
    assert LA.pose_dims("entry", pos, torch.zeros(7, 3)) == (pos.device, 2, 5, 7, 0)
    assert LA.pose_dims("entry", pos, torch.zeros(2, 7, 3)) == (pos.device, 2, 5, 7, 21)
    assert LA.pose_dims("entry", pos, torch.zeros(2, 7, 3), per_sample=True) == (pos.device, 2, 5, 7, 21)
    assert LA.pose_dims("entry", pos[:0], torch.zeros(0, 3)) == (pos.device, 0, 5, 0, 0)
    with pytest.raises(L.DdpError, match="entry: rec"):
        LA.pose_dims("entry", pos, torch.zeros(3, 7, 3))                      # [S + 1, m, 3]
    with pytest.raises(L.DdpError, match="entry: rec .*per sample"):
        LA.pose_dims("entry", pos, torch.zeros(7, 3), per_sample=True)        # a shared receptor given to the per-sample form
    with pytest.raises(L.DdpError, match="entry: rec"):
        LA.pose_dims("entry", pos, torch.zeros(7, 4))
    with pytest.raises(L.DdpError, match="entry pos"):
        LA.pose_dims("entry", pos.double(), torch.zeros(7, 3))
    with pytest.raises(L.DdpError, match="entry: pos"):
        LA.pose_dims("entry", torch.zeros(5, 3), torch.zeros(7, 3))


# ---------------------------------------------------------------------------------------------- 4. the definition at a non-default form
CFG = SC.ScoreConfig(**P.FORM)


def _t(*arrays):
    return [None if a is None else torch.from_numpy(np.asarray(a)) for a in arrays]


def _assert_conditions(x, lig_r, lig_f, rec, rec_r, rec_f):
    assert P.conditions(x, lig_r, lig_f, rec, rec_r, rec_f, P.constants()) == (True, True, True, True)


def test_score_torch_matches_the_restatement_at_a_non_default_form():
    case = P.score_case()
    ref = case[7]
    _assert_conditions(*case[:6])
    assert ref["cutoff_gap"] >= 1e-6 and CFG.check() is CFG
    assert (case[1] < 0).any() and (case[4] < 0).any() and case[0].shape == (2, 37, 3) and case[3].shape == (1025, 3)      # untyped atoms on both sides
    x, lig_r, lig_f, rec, rec_r, rec_f, pairs = _t(*case[:7])
    e, g = SC.score_torch(x, lig_r, lig_f, rec, rec_r, rec_f, pairs, CFG, P.TOR_DIVISOR, with_grad=True)
    be, bg = V.bounds(ref)
    err, eg = np.abs(e.numpy() - ref["energy"]), np.abs(g.numpy() - ref["grad"])
    print("worst |err| / bound: energy", float((err / be).max()), "gradient", float((eg / bg[:, None, None]).max()))
    assert (err <= be).all() and (eg <= bg[:, None, None]).all()
    # the form matters: the defaults and the form with the three zero-default fields rotated both land outside the bound
    for other, want in ((SC.ScoreConfig(), None), (SC.ScoreConfig(**P.SWAPPED), P.score_ref_swapped())):
        e2, _ = SC.score_torch(x, lig_r, lig_f, rec, rec_r, rec_f, pairs, other, P.TOR_DIVISOR)
        assert (np.abs(e2.numpy() - ref["energy"])[:, [0, 2, 3, 4]] > be[:, [0, 2, 3, 4]]).all()
        if want is not None:
            assert (np.abs(e2.numpy() - want["energy"]) <= V.bounds(want)[0]).all()


@pytest.mark.parametrize("n", [37, 70])
def test_profile_torch_matches_the_restatement_at_a_non_default_form(n):
    case = P.profile_case(n)
    ref = case[7]
    _assert_conditions(*case[:6])
    assert ref["threshold_gap"] >= 1e-6
    x, lig_r, lig_f, rec, rec_r, rec_f, ptr = _t(*case[:7])
    prof, bits = IA.profile_torch(x, lig_r, lig_f, rec, rec_r, rec_f, ptr, CFG, I.CONTACT_DISTANCE)
    prof = prof.numpy()
    I.check(prof[..., :4], prof[..., 4], prof[..., 5], prof[..., 6].astype(np.int64), bits.numpy(), ref, f"n={n}")
    assert (prof[..., 6] == np.floor(prof[..., 6])).all()


def test_energy_flex_torch_matches_the_restatement_at_a_non_default_form():
    c = P.flex_case()
    ref = c["ref"]
    _assert_conditions(c["x"], c["lig_r"], c["lig_f"], c["y"], c["rec_r"], c["rec_f"])
    assert ref["cutoff_gap"] >= 1e-6 and F.kink_distance(c, P.constants()) >= 1e-6
    x, y, x0, y0, lig_r, lig_f, rec_r, rec_f, pairs, mov, sc_pairs = _t(*(c[k] for k in ("x", "y", "x0", "y0", "lig_r", "lig_f", "rec_r", "rec_f", "pairs",
                                                                                    "mov", "sc_pairs")))
    e, gx, gy = MF.energy_flex_torch(x, y, x0, y0, lig_r, lig_f, rec_r, rec_f, pairs, mov, sc_pairs, CFG, c["k"], c["k_sc"])
    be, bgx, bgy = F.bounds(ref)
    err = np.abs(e.numpy() - ref["energy"])
    ex, ey = np.abs(gx.numpy() - ref["grad_x"]), np.abs(gy.numpy() - ref["grad_y"])
    print("worst |err| / bound: energy", float((err / be).max()), "dE/dx", float((ex / bgx[:, None, None]).max()), "dE/dy",
          float((ey / bgy[:, None, None]).max()))
    assert (err <= be).all() and (ex <= bgx[:, None, None]).all() and (ey <= bgy[:, None, None]).all()
    assert (ref["energy"][:, :3] != 0).all()
