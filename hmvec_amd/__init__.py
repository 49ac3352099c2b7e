"""hmvec_amd — MI355X-native implementation of hmvec's halo-model power-spectrum hot path.

Drop-in surface (reference: hmvec/__init__.py:1 ``from .hmvec import *``): ``HaloModel`` with
the reference's constructor / ``add_*`` / ``get_power_*`` API, the parameter tables and the
small host helpers users import by name.  The compute path is hand-written HIP behind the
C ABI in ``include/hmgrid.h``; importing this package does not need the GPU library, the
first kernel call does (and fails loudly if it is not built).
"""
from .params import battaglia_defaults, default_params  # noqa: F401
from .cosmology import Cosmology  # noqa: F401
from .background import AnalyticBackground, CambBackground, TabulatedBackground  # noqa: F401
from .halomodel import HaloModel  # noqa: F401
from .functions import *  # noqa: F401,F403  (the reference's free functions, GPU-backed)
from .fft import generic_profile_fft  # noqa: F401  (hmvec/hmvec.py:3 star-imports it into the package)
from .lensing import delta_sigma_nfw, sigma_nfw  # noqa: F401  (cluster lensing: batched projected NFW profiles)
from .gasprofiles import projected_gnfw  # noqa: F401  (projected gas and pressure profiles: Sigma_gas, tau, y)
from .realspace import projected_from_power, xi_from_power  # noqa: F401  (xi(r) and the J0 / J2 transforms of a tabulated spectrum)
from .angular import angular_from_power  # noqa: F401  (w(theta), gamma_t(theta), xi+-(theta): the J0 / J2 / J4 transforms at chi theta, summed over z)
from .angcov import (angular_cov, angular_cov_spectra_device, bin_averaged_bessel, bin_averaged_bessel_device, binned_angular_from_cl,  # noqa: F401
                     binned_angular_from_cl_device, project_cl_cov, project_cl_cov_device, real_cov_gaussian,
                     real_cov_gaussian_device)  # (covariance of the angular correlation functions: Gaussian part, projection of (l, l') matrices)
from .curvedsky import (bin_averaged_wigner, bin_averaged_wigner_device, curved_angular_binned, curved_angular_binned_device,  # noqa: F401
                        curved_angular_cov, curved_angular_cov_device, curved_angular_spectra_device, curved_binned_from_cl,
                        curved_binned_from_cl_device, curved_cov_gaussian, curved_cov_gaussian_device, curved_project_cl_cov,
                        curved_project_cl_cov_device, shear_factor)  # (curved-sky bin-averaged correlation functions and their covariance: Wigner-d weights over integer l)
from .nonlimber import (nonlimber_cl, nonlimber_cl_device, nonlimber_k_rule, nonlimber_transfer,  # noqa: F401
                        nonlimber_transfer_device, refine_gzs, spherical_bessel,
                        spherical_bessel_device)  # (non-Limber angular power spectra of separable sources: spherical Bessel transfer functions per field and their k sum)
from .cov import (GaussianCov, bin_annuli, cl_cov_1halo, cl_cov_ssc, lensing_shape_noise, limber_samples,  # noqa: F401
                  shot_noise, sigma_b_disc)  # (covariances)
from .bispectrum import F2, cl_bispectrum, tree_bispectrum  # noqa: F401  (bispectrum of three tracers)
from .connected import (AngleRule, F3s, angle_rule, cl_cov_connected, connected_trispectrum_device, get_trispectrum, plin_at,  # noqa: F401
                        pt_averages, pt_averages_device, tree_trispectrum)  # (the 2-, 3- and 4-halo terms of the trispectrum and the connected covariance: functions of a model)
from .rsd import legendre_weights, mu_rule, virial_dispersion  # noqa: F401  (redshift-space wedges and multipoles)
from .xipoles import get_xi_multipoles, xi_multipoles_device, xi_multipoles_from_power  # noqa: F401  (redshift-space correlation multipoles xi_0, xi_2, xi_4(s): the j_0 / j_2 / j_4 transforms of P_0, P_2, P_4, of plain arrays and of a model)
from .onepoint import char_exponent, cumulants, lambda_grid, pdf_from_exponent, ring_rule  # noqa: F401  (one-point PDF of a sum of halo profiles)
from .hod_ensemble import central_differences, hod_sets, stencil  # noqa: F401  (HOD parameter ensembles: P_gg, P_gm of many sets)
from . import hod_ensemble  # noqa: F401
from .clusters import (cluster_abundance_device, cluster_cl_cov, cluster_counts_cov, cluster_selection, get_cluster_abundance,  # noqa: F401
                       get_cluster_counts, powerlaw_lnobs, scatter_rule, sz_lnobs)  # (cluster number counts N(z, q) and their covariance: functions of a model)
from .cib import (cib_defaults, cib_luminosities, cib_sed, cl_cib, emission_power_device, emission_tables, get_power_cib,  # noqa: F401
                  register_emission, sed_break, sub_rule)  # (the CIB halo model: multi-frequency spectra, crosses and C_ell: functions of a model)
from . import angcov, angular, bispectrum, cib, clusters, connected, cosmology, cov, curvedsky, fft, functions, gasprofiles, ksz, lensing, nonlimber, onepoint, params, quadrature, realspace, rsd, tinker, utils, xipoles  # noqa: F401
from .functions import __all__ as _fn_all

__all__ = ["HaloModel", "Cosmology", "default_params", "battaglia_defaults", "generic_profile_fft", "sigma_nfw",
           "delta_sigma_nfw", "xi_from_power", "projected_from_power", "angular_from_power", "angular",
           "bin_averaged_bessel", "bin_averaged_bessel_device", "real_cov_gaussian", "real_cov_gaussian_device",
           "binned_angular_from_cl", "binned_angular_from_cl_device", "project_cl_cov", "project_cl_cov_device", "angular_cov",
           "angular_cov_spectra_device", "angcov",
           "bin_averaged_wigner", "bin_averaged_wigner_device", "curved_cov_gaussian", "curved_cov_gaussian_device",
           "curved_binned_from_cl", "curved_binned_from_cl_device", "curved_project_cl_cov", "curved_project_cl_cov_device",
           "shear_factor", "curved_angular_spectra_device", "curved_angular_cov", "curved_angular_cov_device",
           "curved_angular_binned", "curved_angular_binned_device", "curvedsky",
           "spherical_bessel", "spherical_bessel_device", "nonlimber_transfer", "nonlimber_transfer_device", "nonlimber_cl",
           "nonlimber_cl_device", "refine_gzs", "nonlimber_k_rule", "nonlimber",
           "GaussianCov", "bin_annuli", "shot_noise", "lensing_shape_noise", "cl_cov_1halo", "limber_samples", "cov",
           "cl_cov_ssc", "sigma_b_disc",
           "F2", "tree_bispectrum", "cl_bispectrum", "bispectrum",
           "AngleRule", "angle_rule", "plin_at", "F3s", "tree_trispectrum", "pt_averages", "pt_averages_device",
           "connected_trispectrum_device", "get_trispectrum", "cl_cov_connected", "connected",
           "projected_gnfw", "gasprofiles",
           "virial_dispersion", "mu_rule", "legendre_weights", "rsd", "xi_multipoles_from_power", "xi_multipoles_device", "get_xi_multipoles", "xipoles",
           "char_exponent", "cumulants", "pdf_from_exponent", "lambda_grid", "ring_rule", "onepoint",
           "hod_sets", "stencil", "central_differences", "hod_ensemble",
           "cluster_selection", "scatter_rule", "cluster_abundance_device", "get_cluster_abundance", "get_cluster_counts",
           "cluster_counts_cov", "cluster_cl_cov", "sz_lnobs", "powerlaw_lnobs", "clusters",
           "cib_defaults", "sed_break", "cib_sed", "sub_rule", "cib_luminosities", "emission_tables", "emission_power_device",
           "get_power_cib", "cl_cib", "register_emission", "cib",
           "fft", "tinker", "utils", "cosmology", "params"] + list(_fn_all)
