"""The non-default score form and the seeded inputs that tests/test_pose_abi_cpu.py and tests/test_gpu_pose_form.py share: a set of
the eleven constants in which every value differs from ScoreConfig's default and from every other one, and the cases at which each
of the four pose entries is run with it.  Every case is drawn by its reference module AT these constants (so the module's own cutoff
and threshold margins hold for them), is built once, and is checked by `conditions` from the reference side alone: a form whose
ramps no pair sits on, or whose sums are zero, could not tell two constants apart."""
import functools

import numpy as np

import flexmin_ref as F
import interactions_ref as I
import vinardo_ref as V

FORM = dict(cutoff=7.25, gauss_offset=0.3, gauss_width=0.9, hydrophobic_good=0.4, hydrophobic_bad=2.1, hbond_good=-0.8, hbond_bad=0.15,
            w_gauss=-0.05, w_repulsion=0.7, w_hydrophobic=-0.04, w_hbond=-0.55)
# gauss_offset, hydrophobic_good and hbond_bad are all 0 by default: no test at the defaults can tell them apart.  The same form with
# these three rotated among each other (both ramps keep good < bad).
SWAPPED = dict(FORM, gauss_offset=FORM["hydrophobic_good"], hydrophobic_good=FORM["hbond_bad"], hbond_bad=FORM["gauss_offset"])
RESIDUES = (0, 1, 12, 65)      # an empty residue, a single atom, a usual residue, one that needs a second 64-atom chunk
TOR_DIVISOR = 1.0 + V.W_TORSION * 3     # what vinardo_ref.random_case divides by


def constants(form=None) -> V.Constants:
    return V.Constants(**(form or FORM))


def conditions(x, lig_r, lig_f, rec, rec_r, rec_f, c):
    """From the inputs alone, for the ligand-receptor pairs inside the cutoff of the constants c: (every sample has all four sums
    non-zero, some pair lies on the open interval of the hydrophobic ramp, some pair on that of the hbond ramp, some pair has s < 0)."""
    x, rec = np.asarray(x, dtype=np.float64), np.asarray(rec, dtype=np.float64)
    li, rj = np.nonzero(np.asarray(lig_r) >= 0)[0], np.nonzero(np.asarray(rec_r) >= 0)[0]
    ci, cj = (a.reshape(-1) for a in np.meshgrid(li, rj, indexing="ij"))
    fa, fb = np.asarray(lig_f).astype(np.int64)[ci], np.asarray(rec_f).astype(np.int64)[cj]
    hyd = (fa & fb & 1) != 0
    hb = ((((fa >> 1) & (fb >> 2)) | ((fa >> 2) & (fb >> 1))) & 1) != 0
    rsum = np.asarray(lig_r, dtype=np.float64)[ci] + np.asarray(rec_r, dtype=np.float64)[cj]
    sums, on_hyd, on_hb, neg = True, False, False, False
    for s in range(x.shape[0]):
        r = rec[s] if rec.ndim == 3 else rec
        d = np.sqrt(((x[s, ci] - r[cj]) ** 2).sum(-1))
        sd = d - rsum
        inside = d < c.cutoff
        _, t, _, _ = V.pair_terms(x[s, ci] - r[cj], rsum, fa, fb, c)
        sums = sums and bool((t.sum(0) != 0).all())
        on_hyd = on_hyd or bool((inside & hyd & (sd > c.hydrophobic_good) & (sd < c.hydrophobic_bad)).any())
        on_hb = on_hb or bool((inside & hb & (sd > c.hbond_good) & (sd < c.hbond_bad)).any())
        neg = neg or bool((inside & (sd < 0)).any())
    return sums, on_hyd, on_hb, neg


@functools.lru_cache(maxsize=None)
def score_case():
    """S = 2, n = 37 (untyped atoms on both sides), m = 1025 (one full receptor tile and one atom), self pairs: (x, lig_r, lig_f, rec,
    rec_r, rec_f, pairs, ref at FORM)."""
    return V.random_case(2, 37, 1025, seed=1, c=constants())


@functools.lru_cache(maxsize=None)
def score_ref_swapped():
    """vinardo_ref.score of score_case's inputs at SWAPPED (the cutoff is FORM's: the case's cutoff margin holds)."""
    return V.score(*score_case()[:7], TOR_DIVISOR, constants(SWAPPED))


@functools.lru_cache(maxsize=None)
def profile_case(n):
    """S = 2, the residues of RESIDUES: (x, lig_r, lig_f, rec, rec_r, rec_f, res_ptr, ref at FORM)."""
    return I.random_case(2, n, RESIDUES, seed=11 + n, c=constants())


@functools.lru_cache(maxsize=None)
def flex_case():
    """flexmin_ref.random_case(S=2, n=37, m=70, n_mov=9, n_sc=3) drawn and evaluated at FORM."""
    return F.random_case(2, 37, 70, 9, 3, seed=23, c=constants())
