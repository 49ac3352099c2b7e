"""Halo model for kSZ (hmvec/ksz.py): kSZ-tomography reconstruction noise N_vv, its signal-to-noise, the kSZ template
cross-spectrum and the kSZ auto power C_ell (Ma-Fry and its squeezed limit), with the reference's names and
signatures.  Definitions, the quirks kept and the deviations: DESIGN.md section 11.

We use linear matter power for k<0.1 Mpc-1 used in calculations of large-scale Pgv, Pvv and Pgg, and the halo model
for k>0.1 Mpc-1 used in calculations of small-scale Pge, Pee and Pgg (as the reference does).

Three quantities run on the GPU (kernels in hmvec_amd/csrc/kernels/ksz.hpp): the k_S integral of N_vv
(``hmg_ksz_nvv``), the Ma-Fry P_q_perp(k, z) table (``hmg_ksz_pqperp``) and the Limber projection of a P(z, k) table
into C_ell (``hmg_ksz_limber_cl``).  The spectra come from the GPU ``get_power``.  The rest is host numpy on
O(n_mu n_kL) arrays and scalars, as the reference writes it.

The reference gets f(z) and P_lin from CLASS; this package has no CLASS engine, so ``kSZ`` and every function that
builds one take the keyword-only ``accuracy=``, ``background=``, ``ctx=`` and ``device=`` of ``HaloModel``, and the
default engine is ``'camb'``.  ``P_lin_slow`` needs a provider with ``pk_interpolator`` (``TabulatedBackground`` or a
real CAMB).
"""
import warnings

import numpy as np

from . import _native as nat
from ._native import as_device as _dev, context_or_default as _context
from . import utils
from .cosmology import Cosmology
from .halomodel import HaloModel
from .params import default_params

_trapz = getattr(np, "trapezoid", None) or np.trapz

__all__ = ["defaults", "constants", "Ngg", "get_survey_volume", "pge_err_core", "get_kmin", "chi", "ne0_shaw",
           "ksz_radial_function", "kSZ", "Nvv_core_integral", "get_ksz_template_signal_snapshot",
           "get_interpolated_cls", "get_ksz_snr", "get_ksz_auto_signal_mafry", "get_ksz_auto_squeezed", "Nvv"]

defaults = {'min_mass': 1e6, 'max_mass': 1e16, 'num_mass': 1000}
constants = {
    'thompson_SI': 6.6524e-29,
    'meter_to_megaparsec': 3.241e-23,
    'G_SI': 6.674e-11,
    'mProton_SI': 1.673e-27,
    'H100_SI': 3.241e-18
}

_NCHI = 100           # Limber nodes per ell (hmvec/ksz.py:621,835)


def Ngg(ngalMpc3):
    return (1. / ngalMpc3)


def get_survey_volume(zmin, zmax, fsky):
    c = Cosmology(engine='camb', accuracy='low')
    chimin = c.comoving_radial_distance(zmin)
    chimax = c.comoving_radial_distance(zmax)
    return fsky * (4. / 3.) * np.pi * (chimax ** 3. - chimin ** 3.) / 1e9


def pge_err_core(pgv_int, kstar, chistar, volume_gpc3, kss, ks_bin_edges, pggtot, Cls):
    """
    pgv_int: \\int dkl kl^2 Pgv^2/Pggtot
    kstar: kSZ radial weight function at chistar
    chistar: comoving distance to galaxy survey
    volume_gpc3: volume in gpc3
    kss: short wavelength k on which pggtot and cltot are defined
    """
    volume = volume_gpc3 * 1e9
    ints = []
    cltot = get_interpolated_cls(Cls, chistar, kss)
    integrand = (kss / (pggtot * cltot))
    for kleft, kright in zip(ks_bin_edges[:-1], ks_bin_edges[1:]):
        sel = np.s_[np.logical_and(kss > kleft, kss <= kright)]
        y = _sanitize(integrand[sel])
        x = kss[sel]
        ints.append(_trapz(y, x))
    return (volume * kstar ** 2 / 12 / np.pi ** 3 / chistar ** 2. * pgv_int * np.asarray(ints)) ** (-0.5)


def get_kmin(volume_gpc3):
    vol_mpc3 = volume_gpc3 * 1e9
    return np.pi / vol_mpc3 ** (1. / 3.)


def chi(Yp, NHe):
    val = (1 - Yp * (1 - NHe / 4.)) / (1 - Yp / 2.)
    return val


def ne0_shaw(ombh2, Yp, NHe=0, me=1.14, gasfrac=0.9):
    '''
    Average electron density today
    Eq 3 of 1109.0553
    Units: 1/meter**3
    '''
    omgh2 = gasfrac * ombh2
    mu_e = 1.14  # mu_e*mass_proton = mean mass per electron
    ne0_SI = chi(Yp, NHe) * omgh2 * 3. * (constants['H100_SI'] ** 2.) / constants['mProton_SI'] / 8. / np.pi / \
        constants['G_SI'] / mu_e
    return ne0_SI


def ksz_radial_function(z, ombh2, Yp, gasfrac=0.9, xe=1, tau=0, params=None):
    """
    K(z) = - T_CMB sigma_T n_e0 x_e(z) exp(-tau(z)) (1+z)^2
    Eq 4 of 1810.13423
    """
    if params is None:
        params = default_params
    T_CMB_muk = params['T_CMB']  # muK
    thompson_SI = constants['thompson_SI']
    meterToMegaparsec = constants['meter_to_megaparsec']
    ne0 = ne0_shaw(ombh2, Yp)
    return T_CMB_muk * thompson_SI * ne0 * (1. + z) ** 2. / meterToMegaparsec * xe * np.exp(-tau)


def _sanitize(inp):
    inp[~np.isfinite(inp)] = 0
    return inp


def get_interpolated_cls(Cls, chistar, kss):
    """Cls[int(chistar k)] for chistar k <= lmax, inf above; sets Cls[0:2] = 0 in the caller's array, as the reference
    does (hmvec/ksz.py:426-435), vectorised."""
    ls = np.arange(Cls.size)
    Cls[ls < 2] = 0
    ell = chistar * np.asarray(kss)
    inside = ell <= ls[-1]
    idx = np.where(inside, ell, 0).astype(int)
    return np.where(inside, Cls[idx], np.inf).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- device calls
def _cls_array(Cls):
    if not isinstance(Cls, np.ndarray) or Cls.ndim != 1 or Cls.size == 0:
        raise ValueError("Cls must be a non-empty 1-d numpy array starting at l = 0")
    Cls[np.arange(Cls.size) < 2] = 0          # get_interpolated_cls zeroes the caller's array
    return Cls


def _nvv_device(ctx, chis, Fs, mus, kLs, kSs, Cls, Pge, Pgg, ngg, sig=None, H=None, Pph=None, rows=0):
    """Nvv (nz, nmu, nkL) from hmg_ksz_nvv and whether any value is non-finite."""
    ctx = _context(ctx)
    nz, nmu, nkL, nkS = len(chis), mus.size, kLs.size, kSs.size
    d = [_dev(ctx, a) for a in (mus, kLs, kSs, np.asarray(Cls, dtype=np.float64), chis, Fs, ngg, Pge, Pgg)]
    d_sig = _dev(ctx, sig) if sig is not None else None
    d_H = _dev(ctx, H) if H is not None else None
    d_pph = _dev(ctx, Pph) if Pph is not None else None
    out = ctx.empty((nz, nmu, nkL))
    flag = ctx.empty((1,))
    ctx.call("hmg_ksz_nvv", nz, nmu, nkL, nkS, int(Cls.size), rows, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr,
             d[4].ptr, d[5].ptr, d_sig.ptr if d_sig else None, d_H.ptr if d_H else None, d[6].ptr, d[7].ptr,
             d[8].ptr, d_pph.ptr if d_pph else None, out.ptr, flag.ptr)
    bad = bool(flag.numpy().view(np.int32)[0])
    return out.numpy(), bad


def pqperp_table(ks, mus, Pee, Pmm, adotf, *, ctx=None):
    """The Ma-Fry P_q_perp table out[k, z] (hmvec/ksz.py:542-580) for all redshifts in one launch: ks (nk) ascending,
    mus (nmu), Pee and Pmm (nz, nk) paired with ks (either may be a DeviceArray), adotf (nz)."""
    ks = np.ascontiguousarray(ks, dtype=np.float64).ravel()
    mus = np.ascontiguousarray(mus, dtype=np.float64).ravel()
    adotf = np.ascontiguousarray(adotf, dtype=np.float64).ravel()
    nz, nk, nmu = adotf.size, ks.size, mus.size
    if nz == 0 or nk == 0 or nmu == 0:
        raise ValueError("empty grid")
    if nk > 1 and not np.all(np.diff(ks) > 0):
        raise ValueError("ks must be strictly increasing")
    if nmu > 4096:
        raise ValueError("at most 4096 mu nodes")
    for name, a in (("Pee", Pee), ("Pmm", Pmm)):
        if tuple(a.shape if isinstance(a, nat.DeviceArray) else np.shape(a)) != (nz, nk):
            raise ValueError(f"{name} must have shape ({nz}, {nk})")
    ctx = _context(ctx)
    d = [_dev(ctx, a) for a in (ks, mus, Pee, Pmm, adotf)]
    out = ctx.empty((nk, nz))
    ctx.call("hmg_ksz_pqperp", nz, nk, nmu, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, out.ptr)
    return out.numpy()


def limber_cl(ells, chi_nodes, z_nodes, zs, ks, P, squeezed, c2, T2, *, ctx=None):
    """C_ell^kSZ for every ell in one launch (hmvec/ksz.py:596-631 with squeezed=False, 835-862 with True):
    chi_nodes / z_nodes (nell, nchi), P (nk, nz) on (zs, ks), c2 = (sigma_T n_e0 / m->Mpc)^2, T2 = T_CMB^2."""
    ells = np.ascontiguousarray(ells, dtype=np.float64).ravel()
    zs = np.ascontiguousarray(zs, dtype=np.float64).ravel()
    ks = np.ascontiguousarray(ks, dtype=np.float64).ravel()
    nell, nz, nk = ells.size, zs.size, ks.size
    if nz < 2:
        raise ValueError("the C_ell interpolation in (z, k) needs at least two redshifts")
    if nk < 2 or not np.all(np.diff(ks) > 0) or not np.all(np.diff(zs) > 0):
        raise ValueError("zs and ks must be strictly increasing, ks with at least two wavenumbers")
    P = np.asarray(P, dtype=np.float64)
    if P.shape != (nk, nz):
        raise ValueError(f"P must have shape ({nk}, {nz})")
    chi_nodes = np.asarray(chi_nodes, dtype=np.float64)
    z_nodes = np.asarray(z_nodes, dtype=np.float64)
    if chi_nodes.ndim != 2 or chi_nodes.shape[0] != nell or z_nodes.shape != chi_nodes.shape:
        raise ValueError("chi_nodes and z_nodes must be (nell, nchi)")
    if nell == 0:
        return np.zeros(0)
    ctx = _context(ctx)
    d = [_dev(ctx, a) for a in (ells, chi_nodes, z_nodes, zs, ks, P)]
    out = ctx.empty((nell,))
    ctx.call("hmg_ksz_limber_cl", nell, chi_nodes.shape[1], nz, nk, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr,
             d[4].ptr, d[5].ptr, 1 if squeezed else 0, float(c2), float(T2), out.ptr)
    return out.numpy()


def _limber_nodes(pksz, ells, zs):
    """chi = geomspace(ell/30, chi(z_max), 100) per ell and z(chi), for all ells at once (hmvec/ksz.py:618-623)."""
    chi_max = pksz.comoving_radial_distance(zs[-1])
    chi_int = np.geomspace(ells / 30., chi_max, _NCHI, axis=-1)
    z_int = np.asarray(pksz.redshift_at_comoving_radial_distance(chi_int), dtype=np.float64).reshape(chi_int.shape)
    return chi_int, z_int


def _cl_prefactors(pksz):
    """(sigma_T n_e0 / m->Mpc)^2 and T_CMB^2 [muK^2] of hmvec/ksz.py:627-632, from the model's ombh2, YHe and T_CMB
    (the reference's pksz.pars.* do not exist)."""
    ne0 = ne0_shaw(pksz.ombh2, pksz.YHe)
    c2 = (constants['thompson_SI'] * ne0 * 1 / constants['meter_to_megaparsec']) ** 2
    T2 = (pksz.p['T_CMB']) ** 2
    return c2, T2


def _power_on_device(h, name, name2):
    """h.get_power(name, name2) left on the device: the P_1h and P_2h the model holds, added there."""
    ra, rb = h._resolve(name, name if name2 is None else name2)
    h._tsz_notice(ra, rb)
    ent = h._power_cached(ra, rb)
    d1, d2 = ent.p1h, ent.p2h
    ctx = h._ctx()
    out = ctx.empty(d1.shape)
    ctx.call("hmg_add", d1.size, d1.ptr, d2.ptr, out.ptr)
    return out


# ---------------------------------------------------------------------------------------------------- kSZ
class kSZ(HaloModel):
    def __init__(self, zs, volumes_gpc3, ngals_mpc3,
                 kL_max=0.1, num_kL_bins=100, kS_min=0.1, kS_max=10.0,
                 num_kS_bins=101, num_mu_bins=102, ms=None, params=None, mass_function="sheth-torman",
                 halofit=None, mdef='vir', nfw_numeric=False, skip_nfw=False,
                 electron_profile_name='e', electron_profile_family='AGN',
                 skip_electron_profile=False, electron_profile_param_override=None,
                 electron_profile_nxs=None, electron_profile_xmax=None,
                 skip_hod=False, hod_name="g", hod_corr="max", hod_param_override=None,
                 mthreshs_override=None,
                 verbose=False,
                 b1=None, b2=None, sigz=None, engine='camb', *, accuracy='medium', background=None, ctx=None,
                 device=0):

        if ms is None:
            ms = np.geomspace(defaults['min_mass'], defaults['max_mass'], defaults['num_mass'])
        volumes_gpc3 = np.atleast_1d(volumes_gpc3)
        assert len(zs) == len(volumes_gpc3) == len(ngals_mpc3)
        ngals_mpc3 = np.asarray(ngals_mpc3)
        ks = np.geomspace(kS_min, kS_max, num_kS_bins)
        self.ks = ks
        self.mu = np.linspace(-1., 1., num_mu_bins)
        if verbose:
            print('Defining HaloModel')
        HaloModel.__init__(self, zs, ks, ms=ms, params=params, mass_function=mass_function,
                           halofit=halofit, mdef=mdef, nfw_numeric=nfw_numeric, skip_nfw=skip_nfw,
                           accuracy=accuracy, engine=engine, device=device, ctx=ctx, background=background)
        if verbose:
            print('Defining HaloModel: finished')
        self.kS = self.ks
        if not (skip_electron_profile):
            if verbose:
                print('Defining electron profile')
            self.add_battaglia_profile(name=electron_profile_name,
                                       family=electron_profile_family,
                                       param_override=electron_profile_param_override,
                                       nxs=electron_profile_nxs,
                                       xmax=electron_profile_xmax, ignore_existing=False)
            if verbose:
                print('Defining electron profile: finished')

        if not (skip_hod):
            if verbose:
                print('Defining HOD')
            self.add_hod(hod_name, mthresh=mthreshs_override, ngal=ngals_mpc3, corr=hod_corr,
                         satellite_profile_name='nfw',
                         central_profile_name=None, ignore_existing=False, param_override=hod_param_override)
            if verbose:
                print('Defining HOD: finished')

        self.Pmms = []
        self.fs = []
        self.adotf = []
        self.d2vs = []

        self.sigma_z_func = lambda z: sigz * (1. + z)
        self.Hphotozs = self.h_of_z(zs)  # 1/Mpc units

        # Define log-spaced array of k values
        self.kLs = np.geomspace(get_kmin(np.max(volumes_gpc3)), kL_max, num_kL_bins)
        # kr = mu * kL ; this is an array of krs of shape (num_mus,num_kLs)
        self.krs = self.mu.reshape((self.mu.size, 1)) * self.kLs.reshape((1, self.kLs.size))

        self.sigz = sigz
        if not skip_hod:
            self.sPggs = self.get_power(hod_name, name2=hod_name, verbose=verbose, b1=b1, b2=b1)
            self.sPges = self.get_power(hod_name, name2=electron_profile_name, verbose=verbose, b1=b1)
            if sigz is not None:
                oPggs = self.sPggs.copy()
                oPges = self.sPges.copy()
                self.sPggs = []
                self.sPges = []
                for zindex in range(oPggs.shape[0]):
                    self.sPggs.append(oPggs[zindex] * (self.Wphoto(zindex).reshape((self.mu.size, self.kLs.size, 1)) ** 2.))
                    self.sPges.append(oPges[zindex] * (self.Wphoto(zindex).reshape((self.mu.size, self.kLs.size, 1))))
                self.sPggs = np.asarray(self.sPggs)
                self.sPges = np.asarray(self.sPges)

        # Warn user that k_min is the same for all zs
        if np.max(volumes_gpc3) != np.min(volumes_gpc3):
            warnings.warn('Using equal k_min at each z, despite different volumes at each z')

        # get P_linear and f(z) on grid in z and k
        p = self.P_lin_slow(self.kLs, self.zs)
        growth = self.get_growth_rate_f(self.zs)[None, ...]

        self.kstars = []
        self.chistars = []
        self.Vs = volumes_gpc3
        self.vrec = []
        self.sPggtot = []
        self.sPge = []
        self.bgs = []
        # (the unbiased small-scale spectra and shot noise as hmg_ksz_nvv takes them: W is applied on the device)
        self._aPgg, self._aPge, self._ngg = None, None, []
        # (the reference asks for these unconditionally, so skip_hod=True fails here as it does there)
        aPgg = self.get_power('g', 'g', verbose=verbose)
        aPge = self.get_power('g', 'e', verbose=verbose)
        self._aPgg, self._aPge = aPgg, aPge
        for zindex, volume_gpc3 in enumerate(volumes_gpc3):
            self.Pmms.append(np.resize(p[zindex].copy(), (self.mu.size, self.kLs.size)))
            self.fs.append(growth[:, zindex].copy())
            z = self.zs[zindex]
            a = 1. / (1. + z)
            H = self.h_of_z(z)
            self.kstars.append(self.ksz_radial_function(zindex))
            self.d2vs.append(self.fs[zindex] * a * H / self.kLs)
            self.adotf.append(self.fs[zindex] * a * H)

            self.chistars.append(self.comoving_radial_distance(z))

            # Compute P_gg + N_gg and P_gv for fiducial and "true" parameters, as functions of k_L
            bg = self.hods['g']['bg'][zindex]
            self.bgs.append(bg)
            ngal = ngals_mpc3[zindex]
            ngg = Ngg(ngal)
            self._ngg.append(ngg)
            flPgg = self.lPgg(zindex, bg1=bg, bg2=bg)[0, :] + ngg
            flPgv = self.lPgv(zindex, bg=bg)[0, :]
            # Construct integrand (without prefactor) as function of tabulated k_L values, and integrate
            kls = self.kLs
            integrand = _sanitize((kls ** 2.) * (flPgv * flPgv) / flPgg)
            vrec = _trapz(integrand, kls)
            self.vrec.append(vrec.copy())

            if verbose:
                print("Calculating small scale Pgg...")
            Pgg = aPgg[zindex].copy()
            if sigz is not None:
                Pgg = Pgg[None, None] * (self.Wphoto(zindex).reshape((self.mu.size, self.kLs.size, 1)) ** 2.)
            Pggtot = Pgg + ngg
            self.sPggtot.append(Pggtot.copy())
            Pge = aPge[zindex].copy()
            if sigz is not None:
                Pge = Pge[None, None] * (self.Wphoto(zindex).reshape((self.mu.size, self.kLs.size, 1)))
            self.sPge.append(Pge.copy())

        self.ngals_mpc3 = ngals_mpc3

    def Pge_err(self, zindex, ks_bin_edges, Cls):
        kstar = self.kstars[zindex]
        chistar = self.chistars[zindex]
        volume = self.Vs[zindex]
        pgv_int = self.vrec[zindex]
        kss = self.ks
        pggtot = self.sPggtot[zindex][0]
        return pge_err_core(pgv_int, kstar, chistar, volume, kss, ks_bin_edges, pggtot, Cls)

    def lPvv(self, zindex, bv1=1, bv2=1):
        """The long-wavelength power spectrum of vxv: (faH/kL)**2*Pmm(kL), a [mu,kL] array with identical copies over
        mus.  bv1 and bv2 are the velocity biases in each bin."""
        Pvv = (self.d2vs[zindex]) ** 2. * self.Pmms[zindex] * bv1 * bv2
        return Pvv

    def lPgg(self, zindex, bg1, bg2):
        """The long-wavelength power spectrum of gxg; bg1 and bg2 are the linear galaxy biases in each bin."""
        Pgg = self.Pmms[zindex] * bg1 * bg2
        if not (self.sigz is None):
            Pgg = Pgg[..., None] * (self.Wphoto(zindex).reshape((self.mu.size, self.kLs.size, 1)) ** 2.)
        return Pgg

    def lPgv(self, zindex, bg, bv=1):
        """The long-wavelength power spectrum of gxv; bg is the linear galaxy bias, bv the velocity bias."""
        Pgv = self.Pmms[zindex] * bg * bv * (self.d2vs[zindex])
        if not (self.sigz is None):
            Pgv = Pgv[..., None] * (self.Wphoto(zindex).reshape((self.mu.size, self.kLs.size, 1)))
        return Pgv

    def ksz_radial_function(self, zindex, gasfrac=0.9, xe=1, tau=0, params=None):
        return ksz_radial_function(self.zs[zindex], self.ombh2, self.YHe, gasfrac=gasfrac, xe=xe, tau=tau,
                                   params=params)

    def Wphoto(self, zindex):
        krs = self.krs
        z = self.zs[zindex]
        H = self.Hphotozs[zindex]
        return np.exp(-self.sigma_z_func(z) ** 2. * krs ** 2. / 2. / H ** 2.)  # (mus,kLs)

    def Nvv(self, zindex, Cls):
        """N_vv (nmu, nkL) at redshift index zindex: Nvv_core_integral(chi_*, F_*, mu, kL, kS, Cls, sPge, sPggtot)
        as the reference calls it (hmvec/ksz.py:283-292), with the k_S integral on the GPU."""
        return self._nvv([zindex], Cls)[0]

    def _nvv(self, zindices, Cls):
        """N_vv for several redshift indices in one launch: (len(zindices), nmu, nkL)."""
        if self._aPge is None:
            raise ValueError("this kSZ object has no HOD spectra (skip_hod=True)")
        Cls = _cls_array(Cls)
        zi = [int(i) for i in zindices]
        chis = np.array([self.chistars[i] for i in zi], dtype=np.float64)
        Fs = np.array([self.ksz_radial_function(i) for i in zi], dtype=np.float64)
        ngg = np.array([self._ngg[i] for i in zi], dtype=np.float64)
        sig = H = None
        if self.sigz is not None:
            sig = np.array([self.sigma_z_func(self.zs[i]) for i in zi], dtype=np.float64)
            H = np.array([self.Hphotozs[i] for i in zi], dtype=np.float64)
        out, bad = _nvv_device(self._ctx(), chis, Fs, self.mu, self.kLs, self.kS, Cls, self._aPge[zi],
                               self._aPgg[zi], ngg, sig=sig, H=H)
        assert not bad, "non-finite N_vv"
        return out


def Nvv_core_integral(chi_star, Fstar, mu, kL, kSs, Cls, Pge, Pgg_tot, Pgg_photo_tot=None, errs=False,
                      robust_term=False, photo=True, *, ctx=None):
    """
    Returns velocity recon noise Nvv as a function of mu,kL
    Uses Pgg, Pge function of mu,kL,kS and integrates out kS (on the GPU)

    if errs is True: sets Pge=1, so can be reused for Pge error calc

    Cls is an array for C_tot starting at l=0.
    e.g. C_tot = C_CMB + C_fg + (C_noise/beam**2 )
    """
    if robust_term:
        if photo:
            print("WARNING: photo_zs were True for an Nvv(robust_term=True) call. Overriding to False.")
        photo = False

    ret_Pge = None
    if errs:
        ret_Pge = Pge.copy()
        Pge = 1.

    mu = np.asarray(mu, dtype=np.float64).ravel()
    kL = np.asarray(kL, dtype=np.float64).ravel()
    kSs = np.asarray(kSs, dtype=np.float64).ravel()
    if robust_term:
        assert Pgg_photo_tot is not None
    Cls = _cls_array(Cls)
    nkS = kSs.size
    arrs = [np.asarray(Pge, dtype=np.float64), np.asarray(Pgg_tot, dtype=np.float64)]
    if robust_term:
        arrs.append(np.asarray(Pgg_photo_tot, dtype=np.float64))
    full = (mu.size, kL.size, nkS)
    try:
        shape = np.broadcast_shapes(*(a.shape for a in arrs), (nkS,))
        np.broadcast_shapes(shape, full)
    except ValueError:
        raise ValueError(f"Pge, Pgg_tot (and Pgg_photo_tot) must broadcast to (nmu, nkL, nkS) = {full}")
    if len(shape) <= 1:
        rows, arrs = 0, [np.broadcast_to(a, (nkS,))[None] for a in arrs]
    else:
        rows, arrs = 1, [np.broadcast_to(a, full)[None] for a in arrs]
    out, bad = _nvv_device(ctx, np.array([chi_star], dtype=np.float64).ravel(),
                           np.array([Fstar], dtype=np.float64).ravel(), mu, kL, kSs, Cls, arrs[0], arrs[1],
                           np.zeros(1), Pph=arrs[2] if robust_term else None, rows=rows)
    Nvv = out[0]
    assert not bad, "non-finite N_vv"
    if errs:
        return Nvv, ret_Pge
    else:
        return Nvv


def _kwargs_model(accuracy, background, ctx, device):
    return dict(accuracy=accuracy, background=background, ctx=ctx, device=device)


def get_ksz_template_signal_snapshot(ells, volume_gpc3, z, ngal_mpc3, bg, fparams=None, params=None,
                                     kL_max=0.1, num_kL_bins=100, kS_min=0.1, kS_max=10.0,
                                     num_kS_bins=101, num_mu_bins=102, ms=None, mass_function="sheth-torman",
                                     mdef='vir', nfw_numeric=False,
                                     electron_profile_family='AGN',
                                     electron_profile_nxs=None, electron_profile_xmax=None, *,
                                     accuracy='medium', background=None, ctx=None, device=0):
    """
    Get C_ell_That_T, the expected cross-correlation between a kSZ template
    and the CMB temperature.
    """
    mk = _kwargs_model(accuracy, background, ctx, device)
    # Define kSZ object corresponding to fiducial parameters
    fksz = kSZ([z], [volume_gpc3], [ngal_mpc3],
               kL_max=kL_max, num_kL_bins=num_kL_bins, kS_min=kS_min, kS_max=kS_max,
               num_kS_bins=num_kS_bins, num_mu_bins=num_mu_bins, ms=ms, params=fparams, mass_function=mass_function,
               halofit=None, mdef=mdef, nfw_numeric=nfw_numeric, skip_nfw=False,
               electron_profile_name='e', electron_profile_family=electron_profile_family,
               skip_electron_profile=False, electron_profile_param_override=fparams,
               electron_profile_nxs=electron_profile_nxs, electron_profile_xmax=electron_profile_xmax,
               skip_hod=False, hod_name="g", hod_corr="max", hod_param_override=None, **mk)

    # Define kSZ object corresponding to "true" parameters, if specified
    if params is not None:
        pksz = kSZ([z], [volume_gpc3], [ngal_mpc3],
                   kL_max=kL_max, num_kL_bins=num_kL_bins, kS_min=kS_min, kS_max=kS_max,
                   num_kS_bins=num_kS_bins, num_mu_bins=num_mu_bins, ms=ms, params=params,
                   mass_function=mass_function,
                   halofit=None, mdef=mdef, nfw_numeric=nfw_numeric, skip_nfw=False,
                   electron_profile_name='e', electron_profile_family=electron_profile_family,
                   skip_electron_profile=False, electron_profile_param_override=params,
                   electron_profile_nxs=electron_profile_nxs, electron_profile_xmax=electron_profile_xmax, **mk)
    else:
        pksz = fksz

    # Get galaxy shot power as 1/nbar
    ngg = Ngg(ngal_mpc3)

    # Get P_gg + N_gg and P_ge as a function of k_S, for fiducial parameters
    fsPgg = fksz.sPggs[0] + ngg
    fsPge = fksz.sPges[0]

    # Get P_ge as a function of k_S, for "true" parameters
    psPge = pksz.sPges[0] if params is not None else fsPge

    # Get comoving distance to redshift z
    chistar = pksz.comoving_radial_distance(z)

    # P_ge^fid * P_ge^true / P_gg^{tot,fid} at k = ell/chi_* for the specified ells
    iPk = utils.interp(fksz.kS, _sanitize(fsPge * psPge / fsPgg))
    Pks = np.asarray(iPk(np.asarray(ells) / chistar))

    # Get kSZ radial weight function K(z) for fiducial and "true" parameters, at input z
    fFstar = fksz.ksz_radial_function(zindex=0)
    pFstar = pksz.ksz_radial_function(zindex=0) if params is not None else fFstar

    # Get volume in Mpc^3
    V = volume_gpc3 * 1e9

    # Compute prefactor: K^fid K^true V^{1/3} / (6 \pi^2 \chi_*^2)
    pref = fFstar * pFstar * (V ** (1 / 3.)) / 6 / np.pi ** 2 / chistar ** 2

    # Compute P_gg + N_gg and P_gv for fiducial and "true" parameters, as functions of k_L
    flPgg = fksz.lPgg(zindex=0, bg1=bg, bg2=bg)[0, :] + ngg
    flPgv = fksz.lPgv(zindex=0, bg=bg)[0, :]
    plPgv = pksz.lPgv(zindex=0, bg=bg)[0, :] if params is not None else flPgv

    # Construct integrand (without prefactor) as function of tabulated k_L values, and integrate
    kls = fksz.kLs
    integrand = _sanitize((kls ** 2.) * (flPgv * plPgv) / flPgg)
    vrec = _trapz(integrand, kls)

    # Return full integral as function of input ell values, and other info
    return pref * Pks * vrec, fksz, pksz


def get_ksz_snr(volume_gpc3, z, ngal_mpc3, Cls, bg=None, params=None,
                kL_max=0.1, num_kL_bins=100, kS_min=0.1, kS_max=10.0,
                num_kS_bins=101, num_mu_bins=102, ms=None, mass_function="sheth-torman",
                mdef='vir', nfw_numeric=False,
                electron_profile_family='AGN',
                electron_profile_nxs=None, electron_profile_xmax=None, sigz=None, *,
                accuracy='medium', background=None, ctx=None, device=0):
    """
    SNR = \\int 2pi k_L^2 dk_L dmu (1/(2pi)^3) Pgv(mu,kL)^2 / Pggtot(mu,kL)^2 / Nvv(mu,kL)
    """
    fksz = kSZ([z], [volume_gpc3], [ngal_mpc3],
               kL_max=kL_max, num_kL_bins=num_kL_bins, kS_min=kS_min, kS_max=kS_max,
               num_kS_bins=num_kS_bins, num_mu_bins=num_mu_bins, ms=ms, params=params, mass_function=mass_function,
               halofit=None, mdef=mdef, nfw_numeric=nfw_numeric, skip_nfw=False,
               electron_profile_name='e', electron_profile_family=electron_profile_family,
               skip_electron_profile=False, electron_profile_param_override=params,
               electron_profile_nxs=electron_profile_nxs, electron_profile_xmax=electron_profile_xmax,
               skip_hod=False, hod_name="g", hod_corr="max", hod_param_override=None, sigz=sigz,
               **_kwargs_model(accuracy, background, ctx, device))
    V = volume_gpc3 * 1e9
    ngg = Ngg(ngal_mpc3)
    Nvv = fksz.Nvv(0, Cls)
    if bg is None:
        bg = fksz.bgs[0]
    lPgg = fksz.lPgg(zindex=0, bg1=bg, bg2=bg)
    lPgv = fksz.lPgv(zindex=0, bg=bg)
    if sigz is not None:
        lPgg = lPgg[..., 0]
        lPgv = lPgv[..., 0]
    ltPgg = lPgg + ngg
    kls = fksz.kLs
    integrand = _sanitize((kls ** 2.) * (lPgv ** 2) / ltPgg / Nvv)
    result = _trapz(integrand, kls)
    snr2 = _trapz(result, fksz.mu) / (2. * np.pi) ** 2.
    return np.sqrt(V * snr2), fksz


def _debug_meshes(ks, mus, Pee0, Pmm0):
    """The (ik = 0, iz = 0) meshes the reference writes with save_debug_files (hmvec/ksz.py:556-575)."""
    from scipy.interpolate import interp1d
    mu_mesh, k_mesh = np.meshgrid(mus, ks)
    k = ks[0]
    frac = k * (k - 2 * k_mesh * mu_mesh) * (1 - mu_mesh ** 2)
    frac /= (k_mesh ** 2 * (k_mesh ** 2 + k ** 2 - 2 * k * k_mesh * mu_mesh))
    with np.errstate(invalid="ignore", divide="ignore"):
        kmkp = np.sqrt(k_mesh ** 2 + k ** 2 - 2 * k * k_mesh * mu_mesh)
    igr = k_mesh ** 2 * frac
    Pee_mesh = interp1d(ks, Pee0, bounds_error=False, fill_value=0.)(kmkp.flatten()).reshape(kmkp.shape)
    Pmm_mesh = interp1d(ks, Pmm0, bounds_error=False, fill_value=0.)(k_mesh.flatten()).reshape(kmkp.shape)
    igr *= Pmm_mesh * Pee_mesh
    np.savetxt('debug_files/kmkp_mesh.dat', kmkp)
    np.savetxt('debug_files/pee_mesh.dat', Pee_mesh)
    np.savetxt('debug_files/pqperp_igr_mesh.dat', igr)
    np.savetxt('debug_files/pqperp_igr_mu.dat', np.transpose([mus, _trapz(np.nan_to_num(igr), ks, axis=0)]))


def get_ksz_auto_signal_mafry(ells, volume_gpc3, zs, ngal_mpc3, bg, params=None,
                              k_max=100., num_k_bins=200,
                              num_kS_bins=101, num_mu_bins=102, ms=None, mass_function="sheth-torman",
                              mdef='vir', nfw_numeric=False,
                              electron_profile_family='AGN',
                              electron_profile_nxs=None, electron_profile_xmax=None,
                              verbose=False, pksz_in=None, save_debug_files=False, *,
                              accuracy='medium', background=None, ctx=None, device=0):
    """
    Get C_ell_^kSZ, the CMB kSZ auto power, as described by Eq. (B28) and the following
    (unnumbered) equation in Smith et al:

        C_\\ell = \\frac{1}{2} (\\frac{\\sigma_T \\bar{n}_{e,0}}{c})^2
                    \\int \\frac{d\\chi}{\\chi^4 a(\\chi)^2}
                    \\exp(-2\\tau) P_{q_\\perp}(k=\\ell/\\chi, \\chi)

        P_{q_\\perp}(k,z) = \\dot{a}^2 f^2 \\int \\frac{d^3 k'}{(2\\pi)^3}
                            P_{ee}^{NL}(|\\vec{k}-\\vec{k}'|,z)
                            P_{\\delta\\delta}^{lin}(k',z)
                            \\frac{k(k-2k'\\mu')(1-\\mu'^2)}{k'^2(k^2+k'^2-2kk'\\mu}

    C_ell^kSZ is returned in uK^2.  The P_q_perp table (all redshifts) and the C_ell projection (all ells) are one
    GPU launch each.
    """
    # Make sure input redshifts are sorted
    zs = np.sort(np.asarray(zs))
    ells = np.asarray(ells, dtype=np.float64)

    # Make arrays for volume and galaxy number density, for feeding to kSZ object
    volumes_gpc3 = volume_gpc3 * np.ones_like(zs)
    ngals_mpc3 = ngal_mpc3 * np.ones_like(zs)

    if pksz_in is not None:
        pksz = pksz_in
    else:
        if verbose:
            print('Initializing kSZ objects')
        pksz = kSZ(zs, volumes_gpc3, ngals_mpc3,
                   kL_max=k_max, num_kL_bins=num_k_bins, kS_min=get_kmin(volume_gpc3), kS_max=k_max,
                   num_kS_bins=num_k_bins, num_mu_bins=num_mu_bins, ms=ms, params=params,
                   mass_function=mass_function, halofit=None, mdef=mdef, nfw_numeric=nfw_numeric, skip_nfw=False,
                   electron_profile_name='e', electron_profile_family=electron_profile_family,
                   skip_electron_profile=False, electron_profile_param_override=params,
                   electron_profile_nxs=electron_profile_nxs, electron_profile_xmax=electron_profile_xmax,
                   skip_hod=True, verbose=verbose, **_kwargs_model(accuracy, background, ctx, device))

    # Get ks and mus that P_{q_perp} integrand is evaluated at
    ks = pksz.kS
    mus = pksz.mu

    # P_ee as a function of z and k (packed as [z,k]), left on the device
    d_Pee = _power_on_device(pksz, 'e', 'e')

    # P_linear as a function of z and k (packed as [z,k]); the reference pairs it with ks
    Pmm = np.asarray(pksz.Pmms)
    Pmm = Pmm[:, 0, :]
    if Pmm.shape[1] != ks.size:
        raise ValueError("x and y arrays must be equal in length along interpolation axis.")

    if verbose:
        print('Computing P_{q_perp} on grid in k,z')
    adotf = np.array([pksz.adotf[iz][0] for iz in range(zs.shape[0])], dtype=np.float64)
    Pqperp = pqperp_table(ks, mus, d_Pee, Pmm, adotf, ctx=pksz._ctx())

    if save_debug_files:
        sPee = d_Pee.numpy()
        _debug_meshes(ks, mus, sPee[0], Pmm[0])

    if verbose:
        print('Computing C_ell')
    chi_int, z_int = _limber_nodes(pksz, ells, zs)
    c2, T2 = _cl_prefactors(pksz)
    cl = limber_cl(ells, chi_int, z_int, zs, ks, Pqperp, False, c2, T2, ctx=pksz._ctx())

    # If desired, save some files for debugging
    if save_debug_files:
        np.savetxt('debug_files/zs.dat', zs)
        np.savetxt('debug_files/k_invMpc.dat', ks)
        np.savetxt('debug_files/pee.dat', sPee)
        np.savetxt('debug_files/pmm.dat', Pmm)
        np.savetxt('debug_files/pqperp.dat', Pqperp)

    # Return kSZ object (in case we want to use it later) and C_ell array
    return pksz, cl


def get_ksz_auto_squeezed(ells, volume_gpc3, zs, ngals_mpc3, bgs, params=None,
                          k_max=100., num_k_bins=200,
                          num_kS_bins=101, num_mu_bins=102, ms=None, mass_function="sheth-torman",
                          mdef='vir', nfw_numeric=False,
                          electron_profile_family='AGN',
                          electron_profile_nxs=None, electron_profile_xmax=None,
                          verbose=False, pksz_in=None, save_debug_files=False,
                          template=False,
                          ngals_mpc3_for_v=None, *,
                          accuracy='medium', background=None, ctx=None, device=0):
    """
    Get C_ell_^kSZ, the CMB kSZ auto power, as described by the squeezed limit
    in Ma & Fry, with some altered notation:

        C_\\ell = \\int \\frac{d\\chi}{\\chi^2 H_0^2} \\tilde{K}(z[\\chi])^2
                 P_{q_r}(k=\\ell/\\chi, \\chi)

        \\tilde{K}(z) = T_{CMB} \\bar{n}_{e,0} \\sigma_T (1+z)^2 \\exp(-\\tau(z))

        P_{q_r}(k,z) = \\frac{1}{6\\pi^2} \\int dk' (k')^2 P_{vv}(k',z) P_{ee}(k,z)

    C_ell^kSZ is returned in uK^2.  The C_ell projection (all ells) is one GPU launch.
    """
    # Define empty dict for storing spectra
    spec_dict = {}

    # Widen search range for setting lower mass threshold from nbar (on a copy: the caller's dict, or the module's
    # default_params, is left as it was)
    params = dict(default_params if params is None else params)
    params['hod_bisection_search_min_log10mthresh'] = 1

    # Make sure input redshifts are sorted
    zs = np.sort(np.asarray(zs))
    ells = np.asarray(ells, dtype=np.float64)

    # Make arrays for volume, for feeding to kSZ object
    volumes_gpc3 = volume_gpc3 * np.ones_like(zs)

    if ngals_mpc3_for_v is None:
        ngals_mpc3_for_v = ngals_mpc3

    # If not computing for a kSZ template, skip HOD computation to save time
    skip_hod = not template

    if pksz_in is not None:
        pksz = pksz_in
    else:
        if verbose:
            print('Initializing kSZ objects')
        pksz = kSZ(zs, volumes_gpc3, ngals_mpc3,
                   kL_max=k_max, num_kL_bins=num_k_bins, kS_min=get_kmin(volume_gpc3), kS_max=k_max,
                   num_kS_bins=num_k_bins, num_mu_bins=num_mu_bins, ms=ms, params=params,
                   mass_function=mass_function, halofit=None, mdef=mdef, nfw_numeric=nfw_numeric, skip_nfw=False,
                   electron_profile_name='e', electron_profile_family=electron_profile_family,
                   skip_electron_profile=False, electron_profile_param_override=params,
                   electron_profile_nxs=electron_profile_nxs, electron_profile_xmax=electron_profile_xmax,
                   skip_hod=skip_hod, verbose=verbose, b1=bgs, b2=bgs,
                   **_kwargs_model(accuracy, background, ctx, device))

    # Get ks that P_{q_perp} integrand is evaluated at
    ks = pksz.kS
    spec_dict['ks'] = ks

    if not template:
        # P_ee as a function of z and k (packed as [z,k])
        sPee = pksz.get_power('e', name2='e', verbose=False)

        # P_vv as a function of z and k (packed as [z,k])
        lPvv0 = pksz.lPvv(zindex=0)[0, :]
        lPvv = np.zeros((len(zs), lPvv0.shape[0]))
        lPvv[0, :] = lPvv0
        for zi in range(1, len(zs)):
            lPvv[zi, :] = pksz.lPvv(zindex=zi)[0, :]

        spec_dict['sPee'] = sPee
        spec_dict['lPvv'] = lPvv
    else:
        # small-scale P_gg (+ shot noise, in place as the reference does) and P_ge as functions of z and k
        sPgg_for_e = pksz.sPggs
        sPgg_for_v = sPgg_for_e.copy()
        for zi in range(zs.shape[0]):
            sPgg_for_e[zi] += 1 / ngals_mpc3[zi]
            sPgg_for_v[zi] += 1 / ngals_mpc3_for_v[zi]
        sPge = pksz.sPges

        # large-scale P_gv and P_gg as functions of z and k
        lPgv0 = pksz.lPgv(zindex=0, bg=bgs[0])[0, :]
        lPgv = np.zeros((len(zs), lPgv0.shape[0]))
        lPgv[0, :] = lPgv0
        for zi in range(1, len(zs)):
            lPgv[zi, :] = pksz.lPgv(zindex=zi, bg=bgs[zi])[0, :]

        lPgg0 = pksz.lPgg(0, bgs[0], bgs[0])[0, :]
        lPgg = np.zeros((len(zs), lPgg0.shape[0]))
        lPgg[0, :] = lPgg0
        for zi in range(zs.shape[0]):
            lPgg[zi, :] = pksz.lPgg(zi, bgs[zi], bgs[zi])[0, :]
            lPgg[zi] += 1 / ngals_mpc3_for_v[zi]

        spec_dict['sPgg'] = sPgg_for_e
        spec_dict['sPge'] = sPge
        spec_dict['lPgv'] = lPgv
        spec_dict['lPgg'] = lPgg

    # Compute P_{q_r} values on grid in k,z
    if verbose:
        print('Computing P_{q_r} on grid in k,z')
    Pqr = np.zeros((ks.shape[0], zs.shape[0]))
    for zi, z in enumerate(zs):
        kls = pksz.kLs
        if template:
            integrand = _sanitize((kls ** 2.) * lPgv[zi] ** 2 / sPgg_for_v[zi])
        else:
            integrand = _sanitize((kls ** 2.) * lPvv[zi])
        vint = _trapz(integrand, kls)

        if template:
            Pqr[:, zi] = sPge[zi] ** 2 / sPgg_for_e[zi]
        else:
            Pqr[:, zi] = sPee[zi]

        Pqr[:, zi] *= (6 * np.pi ** 2) ** -1 * vint

    if verbose:
        print('Computing C_ell')
    chi_int, z_int = _limber_nodes(pksz, ells, zs)
    c2, T2 = _cl_prefactors(pksz)
    cl = limber_cl(ells, chi_int, z_int, zs, ks, Pqr, True, c2, T2, ctx=pksz._ctx())

    if save_debug_files and not template:
        np.savetxt('debug_files/zs.dat', zs)
        np.savetxt('debug_files/k_invMpc.dat', ks)
        np.savetxt('debug_files/pee.dat', sPee)
        np.savetxt('debug_files/pvv.dat', lPvv)
        np.savetxt('debug_files/pqr.dat', Pqr)

    # Return kSZ object (in case we want to use it later), C_ell array, and dict of spectra used
    return pksz, cl, spec_dict


def Nvv(z, vol_gpc3, ngals_mpc3, Cl_total, sigz=None,
        kL_max=0.1, num_kL_bins=100,
        kS_min=0.1,
        kS_max=10.0,
        num_kS_bins=101,
        num_mu_bins=102, *, accuracy='medium', background=None, ctx=None, device=0):
    """
    Get the reconstruction noise N_vv on the radial velocity field as reconstructed using kSZ tomography using a CMB
    survey and a galaxy survey (hmvec/ksz.py:877-934).

    Returns mus (nmus,), kLs (nkls,) and N_vv (nmus, nkls).
    """
    zs = [z]
    volumes_gpc3 = [vol_gpc3]
    ngals_mpc3 = [ngals_mpc3]
    hksz = kSZ(zs, volumes_gpc3, ngals_mpc3,
               kL_max=kL_max, num_kL_bins=num_kL_bins,
               kS_min=kS_min,
               kS_max=kS_max,
               num_kS_bins=num_kS_bins,
               num_mu_bins=num_mu_bins, sigz=sigz, **_kwargs_model(accuracy, background, ctx, device))
    return hksz.mu, hksz.kLs, hksz.Nvv(0, Cl_total)
