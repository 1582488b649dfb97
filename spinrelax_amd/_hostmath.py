"""
Small host-side (numpy) set-up maths: quantities computed ONCE per run from a handful of numbers
(diffusion-tensor coefficients, the 2592 bin-centre vectors of the Lambert histogram).  Nothing here is
on the hot path; the per-frame / per-residue / per-bin loops are all in the HIP kernels.
"""
import numpy as np


def D_coefficients_symmtop(D):
    """spectral_densities.py:1874-1884: D = (Dpar, Dperp) -> [5Dperp+Dpar, 2Dperp+4Dpar, 6Dperp]."""
    Dpar, Dperp = D[0], D[1]
    return np.array([5 * Dperp + Dpar, 2 * Dperp + 4 * Dpar, 6 * Dperp])


def A_coefficients_symmtop(v, bProlate=True):
    """spectral_densities.py:1886-1906."""
    v = np.asarray(v)
    z2 = np.square(v[..., 2] if bProlate else v[..., 0])
    w = 1 - z2
    return np.stack((3.0 * (z2 * w), 0.75 * np.square(w), 0.25 * np.square(3 * z2 - 1)), axis=-1)


def symmtop_from_iso(Diso, aniso):
    """calculate-relaxations-from-Ct.py:621-622 -> (Dpar, Dperp)."""
    Dperp = 3. * Diso / (2 + aniso)
    return aniso * Dperp, Dperp


# ---- fully anisotropic (rhombic) diffusion: Woessner 1962; Ghose, Fushman & Cowburn 2001 ----
# The reference's helpers of the same names (spectral_densities.py:1908-1932) take sqrt(Diso**2 - D2**2) with D2 already a
# squared quantity: dimensionally inconsistent, and unused by the reference itself.  These follow the physics instead.
def ellipsoid_R(D):
    """R = sqrt(Diso^2 - L^2), L^2 = (DxDy + DxDz + DyDz)/3, as the sum of squared differences it equals (no cancellation
    of two nearly equal squares close to the sphere)."""
    Dx, Dy, Dz = D[0], D[1], D[2]
    return np.sqrt((np.square(Dx - Dy) + np.square(Dx - Dz) + np.square(Dy - Dz)) / 18.0)


def D_coefficients_ellipsoid(D):
    """D = (Dx, Dy, Dz), any order -> the five rates [4Dx+Dy+Dz, Dx+4Dy+Dz, Dx+Dy+4Dz, 6Diso+6R, 6Diso-6R]."""
    Dx, Dy, Dz = float(D[0]), float(D[1]), float(D[2])
    s = Dx + Dy + Dz
    R6 = 6.0 * ellipsoid_R((Dx, Dy, Dz))
    return np.array([s + 3 * Dx, s + 3 * Dy, s + 3 * Dz, 2 * s + R6, 2 * s - R6])


def A_coefficients_ellipsoid(v, D):
    """Amplitudes of the five rates for unit vectors v (..., 3) in the principal-axis frame of D = (Dx, Dy, Dz):
    (..., 5), summing to 1.  delta_i = (D_i - Diso)/R, all zero for the sphere (R == 0)."""
    v = np.asarray(v, dtype=float)
    Dx, Dy, Dz = float(D[0]), float(D[1]), float(D[2])
    Diso = (Dx + Dy + Dz) / 3.0
    R = ellipsoid_R((Dx, Dy, Dz))
    s = 1.0 / (12.0 * R) if R > 0.0 else 0.0
    cx, cy, cz = (Dx - Diso) * s, (Dy - Diso) * s, (Dz - Diso) * s
    x2, y2, z2 = np.square(v[..., 0]), np.square(v[..., 1]), np.square(v[..., 2])
    yz, xz, xy = y2 * z2, x2 * z2, x2 * y2
    x4, y4, z4 = x2 * x2, y2 * y2, z2 * z2
    dd = 0.25 * (3.0 * (x4 + y4 + z4) - 1.0)
    e = cx * (3.0 * x4 + 6.0 * yz - 1.0) + cy * (3.0 * y4 + 6.0 * xz - 1.0) + cz * (3.0 * z4 + 6.0 * xy - 1.0)
    return np.stack((3.0 * yz, 3.0 * xz, 3.0 * xy, dd - e, dd + e), axis=-1)


def J_combine_ellipsoid_exp_decayN(om, v, D, S2, consts, taus):
    """J(om) of C(t) = S2 + sum_k consts_k exp(-t/taus_k) tumbling with the tensor D = (Dx, Dy, Dz), for unit vectors
    v (..., 3) in its principal-axis frame: sum_j A_j [S2 g(d_j, om) + sum_k C_k g(d_j + 1/tau_k, om)], g(x, y) = x/(x^2+y^2).
    Returns (..., len(om)).  Host numpy (set-up sizes and checks); the batched evaluation is model 3 of sr_jomega_relax_f64."""
    om = np.atleast_1d(np.asarray(om, dtype=float))
    dj = D_coefficients_ellipsoid(D)[:, None]
    G = S2 * dj / (dj * dj + om * om)
    for c, t in zip(consts, taus):
        k = dj + 1.0 / t
        G = G + c * k / (k * k + om * om)
    return A_coefficients_ellipsoid(v, D) @ G


def ellipsoid_from_iso(Diso, aniso, rhomb=0.0, unique_z=None):
    """(Diso, aniso, rhomb) -> (Dx, Dy, Dz).  rhomb = 3(Dy - Dx)/(2Dz - Dx - Dy) (ROTDIF) for aniso >= 1; at rhomb = 0 the
    reference's symmetric top: unique axis z for aniso >= 1, x (the reference's oblate convention) below.  unique_z
    (True / False) fixes the unique axis whatever the anisotropy: with it every tensor has a triple."""
    Dperp = 3.0 * Diso / (2.0 + aniso)
    Du = aniso * Dperp
    h = rhomb * (Du - Dperp) / 3.0
    if (aniso >= 1.0) if unique_z is None else unique_z:
        return Dperp - h, Dperp + h, Du
    return Du, Dperp + h, Dperp - h


def iso_from_ellipsoid(D, with_axis=False):
    """(Dx, Dy, Dz) -> (Diso, aniso, rhomb) [, unique_z].  The unique axis is the one of z and x whose value lies farther
    from the mean of the other two (z on a tie, which is rhomb = 1 exactly: both descriptions of such a tensor are
    equivalent), so that |rhomb| <= 1 wherever the tensor allows it.  Inverse of ellipsoid_from_iso for -3 < rhomb < 1;
    for any tensor, ellipsoid_from_iso(Diso, aniso, rhomb, unique_z) gives (Dx, Dy, Dz) back."""
    Dx, Dy, Dz = float(D[0]), float(D[1]), float(D[2])
    Diso = (Dx + Dy + Dz) / 3.0
    unique_z = abs(Dz - 0.5 * (Dx + Dy)) >= abs(Dx - 0.5 * (Dy + Dz))
    if unique_z:
        Du, Dperp, h = Dz, 0.5 * (Dx + Dy), 0.5 * (Dy - Dx)
    else:
        Du, Dperp, h = Dx, 0.5 * (Dy + Dz), 0.5 * (Dy - Dz)
    rhomb = 3.0 * h / (Du - Dperp) if Du != Dperp else 0.0
    if with_axis:
        return Diso, Du / Dperp, rhomb, unique_z
    return Diso, Du / Dperp, rhomb


def rtp_to_xyz_unit(pt):
    """general_maths.py:176-180 (bUnit=True, vaxis=-1): (..., [phi, theta]) -> unit vectors."""
    pt = np.asarray(pt)
    uv = np.zeros(pt.shape[:-1] + (3,), dtype=pt.dtype)
    uv[..., 0] = np.cos(pt[..., 0]) * np.sin(pt[..., 1])
    uv[..., 1] = np.sin(pt[..., 0]) * np.sin(pt[..., 1])
    uv[..., 2] = np.cos(pt[..., 1])
    return uv


def lambert_bin_vectors(edges):
    """spectral_densities.py:2338-2341: bin-centre directions of the (phi, cos theta) histogram,
    flattened phi-major -> (nphi*ncos, 3)."""
    phis = 0.5 * (edges[0][:-1] + edges[0][1:])
    thetas = np.arccos(0.5 * (edges[1][:-1] + edges[1][1:]))
    pt = np.moveaxis(np.array(np.meshgrid(phis, thetas, indexing='ij')), 0, -1)
    bv = rtp_to_xyz_unit(pt)
    return bv.reshape(bv.shape[0] * bv.shape[1], 3)
