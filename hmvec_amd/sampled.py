"""HaloModel's contractions at sample wavenumbers (csrc/sampled.hip; DESIGN.md sections 15, 16, 17): the 1-halo
trispectrum, the bispectrum of three tracers, the response and the super-sample covariance, which share the (nz, n)
sample tables and the way a launch is set up.  The host side of the last three's contract is bispectrum.py and cov.py."""
import ctypes as C

import numpy as np

from . import _native as nat
from . import bispectrum as bispec
from . import cov as covmod
from .spectra import _same_lookups, check_term


def _launch_inputs(h, recs, tables):
    """(ctx, tracers, (d_idx, d_frac, d_scale)); the caller holds on to the uploaded tables until its call is issued."""
    ctx = h._main(needs_aux=True)
    # (another reader of the tensors than the batched mass integrals: a deferred left fill is written first)
    return ctx, [h._tracer(r, 1) for r in recs], h._upload_tables(ctx, tables)


def _launch_kw(h, entry, n, d_tables):
    """What every sampled entry point takes: the grid sizes, the model block (read when the call is made) and the tables."""
    d_idx, d_frac, d_scale = d_tables
    return dict(nz=h._nz, nm=h._nm, nk=h._nk, n=n, **h._model_block(entry), d_idx=d_idx.ptr, d_frac=d_frac.ptr,
                d_scale=d_scale.ptr)


class SampledMixin:
    # ------------------------------------------------------------------ 1-halo trispectrum
    # T[z,i,j] = sum_m wm nzm s_ab[z,m,i] s_cd[z,m,j]: the mass integral of get_power_1halo with one more free index,
    # contracted on the device over the resident tensors (hmg_trispectrum_1h); only (nz, n, n) or (n, n) results cross.
    TRISPECTRUM_MAX_SAMPLES = 1024

    def _sample_tables(self, kindex, idx, frac, scale, damping, max_samples, what):
        """The checked (nz, n) sample tables of a request of `what` ("the trispectrum", ...), which takes at most
        max_samples per redshift: int32 idx, frac, scale (damping=True: folded in).  Everything that can be refused is,
        here, before any launch."""
        nz, nk = self._nz, self._nk
        if idx is None:
            if frac is not None:
                raise ValueError("frac needs idx")
            kindex = np.arange(nk) if kindex is None else np.asarray(kindex)
            if kindex.ndim != 1 or not np.issubdtype(kindex.dtype, np.integer):
                raise ValueError("kindex must be a one-dimensional integer array of indices into ks")
            idx = np.broadcast_to(kindex[None, :], (nz, kindex.size))
        else:
            if kindex is not None:
                raise ValueError("give kindex or the idx / frac tables, not both")
            idx = np.asarray(idx)
            if not np.issubdtype(idx.dtype, np.integer):
                raise ValueError("idx must be an integer array")
            if idx.ndim == 1:
                idx = np.broadcast_to(idx[None, :], (nz, idx.size))
            if idx.ndim != 2 or idx.shape[0] != nz:
                raise ValueError(f"idx must have shape (n,) or (nz, n) with nz = {nz}, got {idx.shape}")
        n = idx.shape[1]
        if n < 1:
            raise ValueError(f"kindex / idx is empty: {what} needs at least one sample")
        if n > max_samples:
            raise ValueError(f"kindex / idx asks for {n} samples per redshift; {what} takes at most {max_samples}: pass "
                             f"a shorter kindex")
        if idx.min() < 0 or idx.max() > nk - 1:
            raise ValueError(f"kindex / idx must lie in 0 .. nk - 1 = {nk - 1}, got {idx.min()} .. {idx.max()}")
        frac = np.zeros((nz, n)) if frac is None else np.broadcast_to(np.asarray(frac, dtype=np.float64), (nz, n))
        if not np.all((frac >= 0.0) & (frac <= 1.0)):
            raise ValueError("frac must lie in [0, 1]")
        if np.any((idx == nk - 1) & (frac != 0.0)):
            raise ValueError("idx = nk - 1 needs frac = 0 (there is no node to its right)")
        scale = np.ones((nz, n)) if scale is None else np.broadcast_to(np.asarray(scale, dtype=np.float64), (nz, n))
        if not np.all(np.isfinite(scale)):
            raise ValueError("scale must be finite")
        if damping:
            ks = self.ks
            k = np.where(frac == 0.0, ks[idx], (1.0 - frac) * ks[idx] + frac * ks[np.minimum(idx + 1, nk - 1)])
            scale = scale * (1.0 - np.exp(-(k / self.p["kstar_damping"]) ** 2.0))
        return (np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(frac, dtype=np.float64),
                np.ascontiguousarray(scale, dtype=np.float64))

    def _trispectrum_tables(self, kindex, idx, frac, scale, damping):
        """_sample_tables of a trispectrum request (the result has nz * n * n entries: at most 1024 samples)."""
        return self._sample_tables(kindex, idx, frac, scale, damping, self.TRISPECTRUM_MAX_SAMPLES, "the trispectrum")

    # what the requests of sections 15, 16, 17 and 19 share
    def _zweights(self, zweights):
        zweights = np.ascontiguousarray(zweights, dtype=np.float64).reshape(-1)
        if zweights.size != self._nz:
            raise ValueError(f"zweights must have one entry per redshift ({self._nz}), got {zweights.size}")
        return zweights

    @staticmethod
    def _upload_tables(ctx, tables):
        """(d_idx, d_frac, d_scale).  They may go back to the free list as soon as the call that reads them is enqueued:
        whatever reuses them is enqueued behind it."""
        return ctx.upload_int32(tables[0]), ctx.upload(tables[1]), ctx.upload(tables[2])

    def trispectrum_device(self, name, name2=None, name3=None, name4=None, kindex=None, damping=True, idx=None,
                           frac=None, scale=None, zweights=None, per_z=True):
        """(T, Tz) on the device: T (nz, n, n) the 1-halo trispectrum of the spectra (name, name2) and (name3, name4) -
        per_z=False: None - and Tz (n, n) = sum_z zweights[z] T[z], in z order, if zweights (nz,) is given, else None.

        Samples: kindex (nodes of ks, the same for every z; default all of them), or tables idx / frac (n,) or (nz, n) -
        sample i of redshift z is the square term interpolated linearly between the nodes idx and idx + 1 at the
        fraction frac (default 0; idx = nk - 1 needs frac = 0), times scale (default 1).  damping=True multiplies scale
        by 1 - exp(-(k / kstar)^2) at the sample's wavenumber, as get_power_1halo damps P_1h.  At most 1024 samples.
        name3 / name4 default to the first pair; the square terms are get_power_1halo's, first-name-only rules
        included."""
        name2 = name if name2 is None else name2
        name3, name4 = (name if name3 is None else name3), (name2 if name4 is None else name4)
        recs = self._resolve(name, name2, name3, name4)
        tables = self._trispectrum_tables(kindex, idx, frac, scale, damping)
        if zweights is not None:
            zweights = self._zweights(zweights)
        elif not per_z:
            raise ValueError("nothing asked for: per_z=False needs zweights")
        nz, n = self._nz, tables[0].shape[1]
        ctx, tr, d_tables = _launch_inputs(self, recs, tables)
        d_g = ctx.upload(zweights) if zweights is not None else None
        T = ctx.empty((nz, n, n)) if per_z else None
        Tz = ctx.empty((n, n)) if zweights is not None else None
        ha, hb, hc, hd = (C.byref(t) for t in tr)
        ctx.call("hmg_trispectrum_1h", h_a=ha, h_b=hb, h_c=hc, h_d=hd, **_launch_kw(self, "hmg_trispectrum_1h", n, d_tables),
                 d_zweights=nat.ptr(d_g), d_T=nat.ptr(T), d_Tz=nat.ptr(Tz))
        self._sync_point()
        return T, Tz

    def get_trispectrum_1halo(self, name, name2=None, name3=None, name4=None, kindex=None, damping=True):
        """1-halo trispectrum T(z; k_i, k_j) = int dm n(z,m) S_ab(z,m,k_i) S_cd(z,m,k_j), shape (nz, n, n), of the spectra
        (name, name2) and (name3, name4; default: the first pair) at the nodes ks[kindex] (default: all; at most 1024).
        S is the square term get_power_1halo integrates, so without damping T[z,i,i] of a pair with itself is the mass
        integral of its square.  damping=True (default) multiplies by D(k_i) D(k_j), D = 1 - exp(-(k/kstar)^2), which
        makes T consistent with the damped P_1h the model returns; damping=False leaves it out."""
        return self.trispectrum_device(name, name2, name3, name4, kindex=kindex, damping=damping)[0].numpy()

    # ------------------------------------------------------------------ bispectrum of three tracers
    # B1h, B2h, B3h at triangles of sample wavenumbers, contracted on the device over the resident tensors
    # (hmg_bispectrum); only (3, nz, nt) or (3, nt) results cross.  The host side of the contract is bispectrum.py.
    def bispectrum_device(self, name, name2=None, name3=None, triangles=None, kindex=None, damping=True, idx=None,
                          frac=None, scale=None, zweights=None, per_z=True):
        """(B, Bz) on the device: B (3, nz, nt) the 1-halo, 2-halo and 3-halo terms of the bispectrum of the tracers
        (name, name2, name3) - per_z=False: None - and Bz (3, nt) = sum_z zweights[z] B[:, z], in z order, if zweights
        (nz,) is given, else None.  Missing names default to the first.

        Samples as for trispectrum_device (kindex, or idx / frac / scale tables; at most 256), except that damping is
        not folded into scale: the factors D = 1 - exp(-(k / kstar)^2) multiply the 1-halo term and the 1-halo factor of
        each 2-halo term.  triangles: (nt, 3) integer array of sample indices, the same for every redshift - leg
        `name` sits at column 0, name2 at 1, name3 at 2; default: all i <= j <= l that close at every redshift; at most
        2^20.  A triangle must close at every redshift.  At most one of the names may be an HOD."""
        return self._bispectrum(name, name2, name3, triangles, kindex, damping, idx, frac, scale, zweights, per_z)[:2]

    def _bispectrum(self, name, name2, name3, triangles, kindex, damping, idx, frac, scale, zweights, per_z, want_J=False):
        """(B, Bz, J) of bispectrum_device; J (3, nz, n), the 2-halo bracket (I + b) - C of each leg at the samples, if
        want_J, else None.  Every refusal happens here on the host, before any launch."""
        name2 = name if name2 is None else name2
        name3 = name if name3 is None else name3
        triple = (name, name2, name3)
        recs = self._resolve(*triple)
        if sum(r.kind1 == "h" for r in recs) >= 2:
            raise NotImplementedError(
                f"bispectrum of {triple!r}: two or more HOD names in one triple need the third factorial moments of the "
                f"HOD for the 1-halo term, which the model does not carry (the product of two galaxy weights would "
                f"count self-pairs)")
        _same_lookups(recs, f"bispectrum of {triple!r}")
        tables = self._sample_tables(kindex, idx, frac, scale, False, bispec.MAX_SAMPLES, "the bispectrum")
        n = tables[0].shape[1]
        tri = bispec.check_triangles(triangles, bispec.sample_wavenumbers(self.ks, tables[0], tables[1]), self.zs)
        if zweights is not None:
            zweights = self._zweights(zweights)
        elif not per_z and not want_J:
            raise ValueError("nothing asked for: per_z=False needs zweights")
        nz, nt = self._nz, tri.shape[0]
        ctx, tr, d_tables = _launch_inputs(self, recs, tables)
        d_tri = ctx.upload_int32(tri)
        d_g = ctx.upload(zweights) if zweights is not None else None
        B = ctx.empty((3, nz, nt)) if per_z else None
        Bz = ctx.empty((3, nt)) if zweights is not None else None
        J = ctx.empty((3, nz, n)) if want_J else None
        ha, hb, hc = (C.byref(t) for t in tr)
        ctx.call("hmg_bispectrum", nt=nt, h_a=ha, h_b=hb, h_c=hc, **_launch_kw(self, "hmg_bispectrum", n, d_tables),
                 kstar=float(self.p["kstar_damping"]) if damping else 0.0, d_tri=d_tri.ptr, d_zweights=nat.ptr(d_g),
                 d_B=nat.ptr(B), d_Bz=nat.ptr(Bz), d_J=nat.ptr(J))
        self._sync_point()
        return B, Bz, J

    def get_bispectrum(self, name, name2=None, name3=None, triangles=None, kindex=None, term="total", damping=True):
        """The halo-model bispectrum B(z; k_1, k_2, k_3) of three tracers (missing names: the first), shape (nz, nt), at
        triangles of the nodes ks[kindex] (default: all nodes; at most 256) - triangles (nt, 3) indexes kindex, leg
        `name` at column 0; default: all i <= j <= l that close.  term: "1h", "2h", "3h" or "total" (their sum in that
        order).  Linear halo bias only (no b_2 term); the 3-halo term uses the tree-level matter bispectrum of the
        model's P_lin.  damping as in get_power_1halo, per leg."""
        check_term(term, bispec.TERMS)
        B = self.bispectrum_device(name, name2, name3, triangles=triangles, kindex=kindex, damping=damping)[0]
        return bispec.pick_term(B.numpy(), term)

    # ------------------------------------------------------------------ response and super-sample covariance (section 17)
    # R_ab = dP_ab / d delta_b at sample wavenumbers for several pairs at once (hmg_response) and the rank-nz contraction
    # Cov = sum_z g r r of such responses (hmg_ssc); only (np, nz, n) and (np n)^2 results cross.  The host side of the
    # contract - sigma_b, the Limber tables, the slope table - is cov.py.
    RESPONSE_MAX_PAIRS = 16

    def _response_request(self, pairs, kindex, idx, frac, scale):
        """(pairs as names, records, tables) of a response request.  Every refusal happens here on the host, before any
        launch."""
        pairs = [(a, a if b is None else b) for a, b in ([p, None] if isinstance(p, str) else p for p in pairs)]
        if len(pairs) < 1:
            raise ValueError("pairs is empty: the response needs at least one (name, name2)")
        if len(pairs) > self.RESPONSE_MAX_PAIRS:
            raise ValueError(f"{len(pairs)} pairs; at most {self.RESPONSE_MAX_PAIRS} are taken in one call")
        recs = self._resolve(*[nm_ for p in pairs for nm_ in p])
        _same_lookups(recs, f"response of {pairs!r}")
        return pairs, recs, self._sample_tables(kindex, idx, frac, scale, False, bispec.MAX_SAMPLES, "the response")

    def _response_launch(self, recs, tables, damping, parts):
        nz, n, npairs = self._nz, tables[0].shape[1], len(recs) // 2
        ctx, tr, d_tables = _launch_inputs(self, recs, tables)
        tr = (nat.Tracer * len(recs))(*tr)
        d_dlnP = self._dev("dlnP", lambda: covmod.dlnp_table(self.ks, self.Pzk))
        R = ctx.empty((npairs, nz, n))
        P = ctx.empty((3, npairs, nz, n)) if parts else None
        ctx.call("hmg_response", np=npairs, h_pairs=tr, **_launch_kw(self, "hmg_response", n, d_tables),
                 d_dlnP=d_dlnP.ptr, kstar=float(self.p["kstar_damping"]) if damping else 0.0, d_R=R.ptr,
                 d_parts=nat.ptr(P))
        self._sync_point()
        return R, P

    def response_device(self, pairs, kindex=None, damping=True, idx=None, frac=None, scale=None, parts=False):
        """R on the device, (np, nz, n): the response dP_ab / d delta_b of the halo-model spectrum of each pair (a, b) of
        `pairs` (1 to 16; a lone name or (a, None) is (a, a)) to a long-wavelength density mode,

            R = scale [ (47/21 - n_s/3) P2h + D I1 - (beta_a + beta_b) (P2h + D A1) ],

        A1 the undamped 1-halo integral of get_power_1halo (first-name-only rules included), I1 the same integral weighted
        with the halo bias, P2h = P_lin J_a J_b the 2-halo term of get_power_2halo, n_s the logarithmic slope of P_lin,
        D the damping factor of get_power_1halo (damping=False: 1) and beta the mean galaxy bias of an HOD name (0 of a
        matter or pressure name: a galaxy overdensity is defined against the local mean density).  The growth and
        dilation factor takes the slope of P_lin only, not of the 2-halo brackets - the usual halo-model approximation.
        Samples as for bispectrum_device (kindex, or idx / frac / scale tables; at most 256).  parts=True: (R, parts),
        parts (3, np, nz, n) = (A1, I1, P2h), unscaled and undamped.  Two HOD names in one pair are allowed."""
        _, recs, tables = self._response_request(pairs, kindex, idx, frac, scale)
        R, P = self._response_launch(recs, tables, damping, parts)
        return (R, P) if parts else R

    def get_power_response(self, name, name2=None, kindex=None, damping=True):
        """dP_ab(z, k) / d delta_b of the pair (name, name2; default name) at the nodes ks[kindex] (default: all, at most
        256), shape (nz, n); see response_device."""
        return self.response_device([(name, name2)], kindex=kindex, damping=damping).numpy()[0]

    def ssc_device(self, pairs, zweights, zscale=None, kindex=None, damping=True, idx=None, frac=None, scale=None):
        """Cov on the device, (np, n, np, n): Cov[p,i,q,j] = sum_z zweights[z] r[p,z,i] r[q,z,j], in z order, of the
        responses r[p,z,s] = zscale[p][z] R_p[z,s] (response_device's; zscale (np, nz), default 1).  Each term is formed
        as fma(r r, g, acc) with the weight on neither side: Cov[p,i,q,j] has the bits of Cov[q,j,p,i]."""
        pairs, recs, tables = self._response_request(pairs, kindex, idx, frac, scale)
        nz, n, npairs = self._nz, tables[0].shape[1], len(pairs)
        zweights = np.ascontiguousarray(zweights, dtype=np.float64)
        if zweights.shape != (nz,):
            raise ValueError(f"zweights must have one entry per redshift ({nz}), got shape {zweights.shape}")
        if zscale is not None:
            zscale = np.ascontiguousarray(zscale, dtype=np.float64)
            if zscale.shape != (npairs, nz):
                raise ValueError(f"zscale must have shape (np, nz) = {(npairs, nz)}, got {zscale.shape}")
        R, _ = self._response_launch(recs, tables, damping, False)
        return self._ssc_launch(R, zweights, zscale)

    def _ssc_launch(self, R, zweights, zscale):
        npairs, nz, n = R.shape
        ctx = self._main()
        d_g = ctx.upload(zweights)
        d_zs = ctx.upload(zscale) if zscale is not None else None
        cov_ = ctx.empty((npairs, n, npairs, n))
        ctx.call("hmg_ssc", nz, n, npairs, R.ptr, nat.ptr(d_zs), d_g.ptr, cov_.ptr)
        self._sync_point()
        return cov_
