"""Resource table of the kernels a pass launches: registers, scratch reservation, occupancy and
- the part the compiler's summary does not tell - how many scratch INSTRUCTIONS and SGPR-spill lane moves the ISA
holds and where.  Reads the .resources.txt and .s files of hmgrid.hip, longgrid.hip, lensing.hip, ksz.hip, realspace.hip, hankel.hip, angcov.hip, curvedsky.hip, nonlimber.hip, trispectrum.hip, bispectrum.hip, response.hip, connected.hip, gasproj.hip, rsd.hip, onepoint.hip, hodens.hip, clusters.hip, cib.hip and sampled.hip (`make -C hmvec_amd/csrc asm`).
Usage: python tools/kernel_resources.py > profiles/rNN/kernel_resources.txt"""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(HERE, "hmvec_amd", "csrc")
sys.path.insert(0, HERE)
KERNELS = [   # (label, regex on the mangled name)
    ("front_group_kernel<2>  (nz > 16)", r"front_group_kernelILi2E"),
    ("front_group_kernel<1>  (nz <= 16)", r"front_group_kernelILi1E"),
    ("tensor_group_kernel<2,3,2500,2>  (nxs = 5000: chain | profile rows | NFW rows two per workgroup, the launch of a pass on a full grid)", r"tensor_group_kernelILi2ELi3ELi2500ELi2EE"),
    ("tensor_group_kernel<2,3,2500,1>  (the same with one NFW row per workgroup: thin slabs)", r"tensor_group_kernelILi2ELi3ELi2500ELi1EE"),
    ("rows_group_kernel  (HMG_NO_TENSOR_GROUP=1, and passes without a profile transform)", r"17rows_group_kernelE"),
    ("profile_group_kernel<2,3,2500>  (nxs = 5000; a second profile of a pass, HMG_NO_TENSOR_GROUP=1)", r"profile_group_kernelILi2ELi3ELi2500E"),
    ("power_batch_kernel<2,3,2,false,593,true>  (Config 3, full grid: the NFW tensor in the series slot)", r"power_batch_kernelILi2ELi3ELi2ELb0ELj593ELb1E"),
    ("power_batch_kernel<2,3,1,false,593,true>  (the same for an odd nk)", r"power_batch_kernelILi2ELi3ELi1ELb0ELj593ELb1E"),
    ("power_batch_kernel<2,3,1,true,593,true>  (thin slab, 64-k tiles, series slot)", r"power_batch_kernelILi2ELi3ELi1ELb1ELj593ELb1E"),
    ("power_batch_kernel<2,3,2,true,593,true>  (thin slab, 128-k tiles, series slot)", r"power_batch_kernelILi2ELi3ELi2ELb1ELj593ELb1E"),
    ("power_batch_kernel<2,3,2,false,593>  (Config 3, full grid, tensors written whole)", r"power_batch_kernelILi2ELi3ELi2ELb0ELj593ELb0E"),
    ("power_batch_kernel<2,3,1,true,593>  (thin slab)", r"power_batch_kernelILi2ELi3ELi1ELb1ELj593ELb0E"),
    ("nfw_series_fill_kernel  (fill of a deferred short-series band)", r"22nfw_series_fill_kernelE"),
    ("profile_pruned_kernel<512,1000>  (nxs = 30000)", r"profile_pruned_kernelILi512ELi1000E"),
    ("profile_pruned_kernel<512,1250>  (nxs = 40000)", r"profile_pruned_kernelILi512ELi1250E"),
    ("profile_band_kernel<512,1000,1>  (tSZ: nxs = 30000, xmax = 2, <= 255 modes)", r"profile_band_kernelILi512ELi1000ELi1E"),
    ("profile_band_kernel<512,1000,2>  (the same, up to 499 modes)", r"profile_band_kernelILi512ELi1000ELi2E"),
    ("profile_group_kernel<1,2,1500>  (nxs = 3000, compile-time plan, round 5)", r"profile_group_kernelILi1ELi2ELi1500E"),
    ("profile_group_kernel<3,3,3000>  (nxs = 6000 as one row, round 5)", r"profile_group_kernelILi3ELi3ELi3000E"),
    ("profile_group_kernel<2,3,0>  (run-time plan)", r"profile_group_kernelILi2ELi3ELi0E"),
    ("profile_table_kernel<512,2,3,2500>  (user callable, nxs = 5000, round 5)", r"profile_table_kernelILi512ELi2ELi3ELi2500E"),
    ("profile_table_kernel<512,2,4,0>  (user callable, run-time plan)", r"profile_table_kernelILi512ELi2ELi4ELi0E"),
    ("stand-alone: profile_fused_kernel<512,2,3,2500>", r"profile_fused_kernelILi512ELi2ELi3ELi2500E"),
    ("stand-alone: nfw_kernel", r"10nfw_kernelE"),
    ("lensing_centred_kernel<false>  (centred Sigma, lensing.hip)", r"22lensing_centred_kernelILb0EE"),
    ("lensing_off_kernel<4,false>  (miscentred Sigma, lensing.hip)", r"18lensing_off_kernelILi4ELb0EE"),
    ("lensing_2h_kernel<256,0>  (two-halo convergence, lensing.hip)", r"17lensing_2h_kernelILi256ELi0EE"),
    ("lensing_centred_kernel<true>  (centred Delta Sigma, lensing.hip)", r"22lensing_centred_kernelILb1EE"),
    ("lensing_off_kernel<4,true>  (miscentred Delta Sigma, lensing.hip)", r"18lensing_off_kernelILi4ELb1EE"),
    ("lensing_2h_kernel<256,2>  (two-halo tangential shear, lensing.hip)", r"17lensing_2h_kernelILi256ELi2EE"),
    ("ksz_pqperp_kernel<true>  (P_q_perp, tables in LDS, ksz.hip)", r"17ksz_pqperp_kernelILb1EE"),
    ("ksz_pqperp_kernel<false>  (P_q_perp, tables from memory, ksz.hip)", r"17ksz_pqperp_kernelILb0EE"),
    ("ksz_nvv_shared_kernel  (N_vv, one k_S integral per z, ksz.hip)", r"21ksz_nvv_shared_kernelE"),
    ("ksz_nvv_rows_kernel  (N_vv, photo-z / per-row, ksz.hip)", r"19ksz_nvv_rows_kernelE"),
    ("ksz_limber_cl_kernel  (kSZ C_ell, ksz.hip)", r"20ksz_limber_cl_kernelE"),
    ("xi_multipole_kernel<256,4,true,false,false,true>  (xi(r): hmg_xi_transform, order 0 with node_stride 1 at compile time; realspace.hip)", r"19xi_multipole_kernelILi256ELi4ELb1ELb0ELb0ELb1EE"),
    ("xi_multipole_kernel<256,4,true,false,false,false>  (xi_0; realspace.hip)", r"19xi_multipole_kernelILi256ELi4ELb1ELb0ELb0ELb0EE"),
    ("xi_multipole_kernel<256,4,false,true,false,false>  (xi_2; realspace.hip)", r"19xi_multipole_kernelILi256ELi4ELb0ELb1ELb0ELb0EE"),
    ("xi_multipole_kernel<256,4,true,true,false,false>  (xi_0 and xi_2; realspace.hip)", r"19xi_multipole_kernelILi256ELi4ELb1ELb1ELb0ELb0EE"),
    ("xi_multipole_kernel<256,4,false,false,true,false>  (xi_4; realspace.hip)", r"19xi_multipole_kernelILi256ELi4ELb0ELb0ELb1ELb0EE"),
    ("xi_multipole_kernel<256,4,true,false,true,false>  (xi_0 and xi_4; realspace.hip)", r"19xi_multipole_kernelILi256ELi4ELb1ELb0ELb1ELb0EE"),
    ("xi_multipole_kernel<256,4,false,true,true,false>  (xi_2 and xi_4; realspace.hip)", r"19xi_multipole_kernelILi256ELi4ELb0ELb1ELb1ELb0EE"),
    ("xi_multipole_kernel<256,4,true,true,true,false>  (all three multipoles; realspace.hip)", r"19xi_multipole_kernelILi256ELi4ELb1ELb1ELb1ELb0EE"),
    ("angular_transform_kernel<256,4,true,false,false,PlainRadius>  (W_0: w_p, Sigma at given radii, hmg_hankel_transform; hankel.hip)", r"24angular_transform_kernelILi256ELi4ELb1ELb0ELb0ENS_11PlainRadiusEE"),
    ("angular_transform_kernel<256,4,false,true,false,PlainRadius>  (W_2: Delta Sigma at given radii, hmg_hankel_transform; hankel.hip)", r"24angular_transform_kernelILi256ELi4ELb0ELb1ELb0ENS_11PlainRadiusEE"),
    ("angular_transform_kernel<256,4,true,true,false,PlainRadius>  (W_0 and W_2 from one pass at given radii, hmg_hankel_transform; hankel.hip)", r"24angular_transform_kernelILi256ELi4ELb1ELb1ELb0ENS_11PlainRadiusEE"),
    ("angular_transform_kernel<256,4,true,false,false,ChiThetaRadius>  (W_0: w(theta), xi+, hmg_angular_transform; hankel.hip)", r"24angular_transform_kernelILi256ELi4ELb1ELb0ELb0ENS_14ChiThetaRadiusEE"),
    ("angular_transform_kernel<256,4,false,true,false,ChiThetaRadius>  (W_2: gamma_t, hmg_angular_transform; hankel.hip)", r"24angular_transform_kernelILi256ELi4ELb0ELb1ELb0ENS_14ChiThetaRadiusEE"),
    ("angular_transform_kernel<256,4,true,true,false,ChiThetaRadius>  (W_0 and W_2, hmg_angular_transform; hankel.hip)", r"24angular_transform_kernelILi256ELi4ELb1ELb1ELb0ENS_14ChiThetaRadiusEE"),
    ("angular_transform_kernel<256,4,false,false,true,ChiThetaRadius>  (W_4: xi-, hmg_angular_transform; hankel.hip)", r"24angular_transform_kernelILi256ELi4ELb0ELb0ELb1ENS_14ChiThetaRadiusEE"),
    ("angular_transform_kernel<256,4,true,false,true,ChiThetaRadius>  (W_0 and W_4: xi+ and xi-, hmg_angular_transform; hankel.hip)", r"24angular_transform_kernelILi256ELi4ELb1ELb0ELb1ENS_14ChiThetaRadiusEE"),
    ("angular_transform_kernel<256,4,false,true,true,ChiThetaRadius>  (W_2 and W_4, hmg_angular_transform; hankel.hip)", r"24angular_transform_kernelILi256ELi4ELb0ELb1ELb1ENS_14ChiThetaRadiusEE"),
    ("angular_transform_kernel<256,4,true,true,true,ChiThetaRadius>  (all three orders, hmg_angular_transform; hankel.hip)", r"24angular_transform_kernelILi256ELi4ELb1ELb1ELb1ENS_14ChiThetaRadiusEE"),
    ("angular_zsum_kernel  (the z sum of the angular transforms, hankel.hip)", r"19angular_zsum_kernelE"),
    ("angcov_weights_kernel  (bin-averaged Bessel weights K_0, K_2, K_4; angcov.hip)", r"21angcov_weights_kernelE"),
    ("angcov_gaussian_kernel<false>  (Gaussian covariance of angular correlation functions, 32 x 32 bins per wavefront; angcov.hip)", r"22angcov_gaussian_kernelILb0EE"),
    ("angcov_combine_kernel<false>  (its chunks' sums in order, the transpose and the noise term; angcov.hip)", r"21angcov_combine_kernelILb0EE"),
    ("angcov_node_weights_kernel<false>  (node weights R_mu; angcov.hip)", r"26angcov_node_weights_kernelILb0EE"),
    ("angcov_gaussian_kernel<true>  (the same contraction with the curved-sky measure l + 1/2 and four kinds; angcov.hip)", r"22angcov_gaussian_kernelILb1EE"),
    ("angcov_combine_kernel<true>  (its combine with the spherical noise term; angcov.hip)", r"21angcov_combine_kernelILb1EE"),
    ("angcov_node_weights_kernel<true>  (curved-sky node weights R_kind; angcov.hip)", r"26angcov_node_weights_kernelILb1EE"),
    ("curvedsky_weights_kernel  (bin-averaged Wigner-d weights of four kinds, one thread per edge; curvedsky.hip)", r"24curvedsky_weights_kernelE"),
    ("curvedsky_scale_kernel  (shear factors of a node table; curvedsky.hip)", r"22curvedsky_scale_kernelE"),
    ("nonlimber_transfer_kernel  (non-Limber transfer functions: one k node per workgroup, 256 chi nodes per chunk, tiles of 16 orders through LDS; nonlimber.hip)", r"25nonlimber_transfer_kernelE"),
    ("sph_bessel_kernel  (j_0 .. j_lmax at one argument per thread; nonlimber.hip)", r"17sph_bessel_kernelE"),
    ("nonlimber_cl_kernel  (the k sum, one wavefront per (pair, l); nonlimber.hip)", r"19nonlimber_cl_kernelE"),
    ("trispectrum_1h_kernel  (1-halo trispectrum, 64 x 64 tile, trispectrum.hip)", r"21trispectrum_1h_kernelE"),
    ("bispectrum_kernel  (bispectrum of three tracers, 1024 triangles per workgroup, bispectrum.hip)", r"17bispectrum_kernelE"),
    ("bispectrum_check_kernel  (its table and triangle check, bispectrum.hip)", r"23bispectrum_check_kernelE"),
    ("response_pairs_kernel  (response of halo-model spectra to a long mode: A1, I1 and the epilogue, response.hip)", r"21response_pairs_kernelE"),
    ("ssc_kernel  (super-sample contraction, 64 x 64 tile, response.hip)", r"10ssc_kernelE"),
    ("pt_average_kernel  (angle-averaged PT matrices Pbar, Bbar, Tbar, one thread per (z, i <= j), dynamic LDS 8 (2 nk + 4 nr) B, connected.hip)", r"17pt_average_kernelE"),
    ("connected_kernel  (2-, 3- and 4-halo terms of the trispectrum, 32 x 32 tile, 2 x 2 register block, connected.hip)", r"16connected_kernelE"),
    ("gnfw_projected_kernel  (projected gas / pressure profile: Sigma, mean, excess; gasproj.hip)", r"21gnfw_projected_kernelE"),
    ("gnfw_smooth_kernel<4>  (the projection through a Gaussian beam, gasproj.hip)", r"18gnfw_smooth_kernelILi4EE"),
    ("rsd_wedge_kernel<true>  (redshift-space wedges P1h, P2h, 8 nodes of mu per thread, rsd.hip)", r"16rsd_wedge_kernelILb1EE"),
    ("rsd_wedge_kernel<false>  (the 2-halo wedge alone, for the multipoles, rsd.hip)", r"16rsd_wedge_kernelILb0EE"),
    ("rsd_multipole_kernel  (1-halo multipoles from the Gaussian moments, rsd.hip)", r"20rsd_multipole_kernelE"),
    ("rsd_contract_kernel  (2-halo multipoles: the rule's sum over mu, rsd.hip)", r"19rsd_contract_kernelE"),
    ("rsd_check_kernel  (its table check, rsd.hip)", r"16rsd_check_kernelE"),
    ("onepoint_exponent_kernel  (exponent of the one-point characteristic function, one lambda per lane, onepoint.hip)", r"24onepoint_exponent_kernelE"),
    ("onepoint_moments_kernel  (cumulants of the one-point PDF, onepoint.hip)", r"23onepoint_moments_kernelE"),
    ("onepoint_finish_kernel  (the sum over slices and over z, onepoint.hip)", r"22onepoint_finish_kernelE"),
    ("hodens_power_kernel<8,true>  (HOD ensemble contraction, 8 sets per thread, one tensor for both legs, hodens.hip)", r"19hodens_power_kernelILi8ELb1EE"),
    ("hodens_power_kernel<8,false>  (the same with a matter tensor of its own, hodens.hip)", r"19hodens_power_kernelILi8ELb0EE"),
    ("hodens_power_kernel<2,true>  (fewer than 256 columns: 2 sets per thread, hodens.hip)", r"19hodens_power_kernelILi2ELb1EE"),
    ("hodens_power_kernel<2,false>  (the same with a matter tensor of its own, hodens.hip)", r"19hodens_power_kernelILi2ELb0EE"),
    ("hodens_occ_kernel  (occupations, n_gal, b_g and the coefficient block of an HOD ensemble, hodens.hip)", r"17hodens_occ_kernelE"),
    ("hodens_lmstar_kernel  (the SHMR inversion, once per (z, m), hodens.hip)", r"20hodens_lmstar_kernelE"),
    ("hodens_side_kernel  (the side data of the mass bins, hodens.hip)", r"18hodens_side_kernelE"),
    ("hodens_check_kernel  (the check of a node list, hodens.hip)", r"19hodens_check_kernelE"),
    ("cluster_selection_kernel  (cluster counts: the selection of a 64-mass tile in up to 8 bins and its mass sum, clusters.hip)", r"24cluster_selection_kernelE"),
    ("cluster_finish_kernel  (the tiles' sums in order, clusters.hip)", r"21cluster_finish_kernelE"),
    ("cib_luminosity_kernel  (CIB: L_c and L_s of a halo at every frequency, one wavefront per (z, m), cib.hip)", r"21cib_luminosity_kernelE"),
    ("emission_power_kernel<0>  (CIB contraction, a 4 x 4 tile of frequency pairs per thread, no partner, cib.hip)", r"21emission_power_kernelILi0EE"),
    ("emission_power_kernel<1>  (the same with one partner, cib.hip)", r"21emission_power_kernelILi1EE"),
    ("emission_power_kernel<2>  (the same with two partners, cib.hip)", r"21emission_power_kernelILi2EE"),
    ("emission_prep_kernel  (the frequency-padded coefficients and the side data of the mass bins, cib.hip)", r"20emission_prep_kernelE"),
    ("emission_check_kernel  (the check of a node list, cib.hip)", r"21emission_check_kernelE"),
    ("leg_prepass_kernel  (leg prepass of the bispectrum and the response: I, C, b, J, P, D, k at the samples, sampled.hip)", r"18leg_prepass_kernelE"),
    ("leg_sums_kernel  (C, C0, b of a leg, for the response and the redshift-space spectra, sampled.hip)", r"15leg_sums_kernelE"),
    ("zsum_kernel  (the z sum of the trispectrum and the bispectrum, sampled.hip)", r"11zsum_kernelE"),
    ("sample_check_kernel  (the table check of the trispectrum and the response, sampled.hip)", r"19sample_check_kernelE"),
]


def main():
    if "--no-build" not in sys.argv:
        subprocess.run(["make", "-j2", "-B", "-C", CSRC, "asm"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    units = ("hmgrid", "longgrid", "lensing", "ksz", "realspace", "hankel", "angcov", "curvedsky", "nonlimber", "trispectrum", "bispectrum", "response", "connected", "gasproj", "rsd", "onepoint", "hodens", "clusters", "cib", "sampled")
    res = "".join(open(os.path.join(CSRC, u + ".resources.txt")).read() for u in units)
    asm = "".join(open(os.path.join(CSRC, u + ".s")).read() for u in units)
    from hmvec_amd._native import kernel_source_sha16
    print(f"# kernel sources {kernel_source_sha16()}  (hipcc -O3 --offload-arch=gfx950 -mllvm -disable-machine-licm; make asm)")
    print("# columns: SGPRs VGPRs | LDS B/workgroup | reserved scratch B/lane | occupancy waves/SIMD | SGPR spills, VGPR spills (compiler summary) |")
    print("#          scratch_* instructions in the ISA | v_writelane/v_readlane (SGPR spills live in VGPR lanes, not in memory)")
    for label, pat in KERNELS:
        m = re.search(r"Function Name: (_ZN3hmg\d*" + pat + r"\S*)(.*?)LDS Size \[bytes/block\]: (\d+)", res, re.S)
        if not m:
            print(f"{label}: not found")
            continue
        name, block, lds = m.group(1), m.group(2), m.group(3)
        g = lambda key: re.search(key + r": (\d+)", block).group(1)      # noqa: E731
        body = asm[asm.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        lines = body.splitlines()
        scr = [i for i, l in enumerate(lines) if re.match(r"\s*scratch_", l)]
        wl = sum(1 for l in lines if re.match(r"\s*v_writelane", l))
        rl = sum(1 for l in lines if re.match(r"\s*v_readlane", l))
        scratch, occ = g(r"ScratchSize \[bytes/lane\]"), g(r"Occupancy \[waves/SIMD\]")
        where = (", at lines " + ",".join(map(str, scr))) if scr else ""
        print(f"{label}\n    SGPRs {g('TotalSGPRs')}  VGPRs {g('VGPRs')} | LDS {lds} B | scratch {scratch} B | occupancy {occ} | spills: SGPR "
              f"{g('SGPRs Spill')}, VGPR {g('VGPRs Spill')} | scratch instructions {len(scr)} (of {len(lines)} lines{where}) | "
              f"lane moves {wl}/{rl}")


if __name__ == "__main__":
    main()
