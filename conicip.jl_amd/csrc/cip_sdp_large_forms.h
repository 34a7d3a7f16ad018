// Which form of each stage an S cone of order 133 .. 2048 runs (sdp_large.hip, sdp_large_nt.hip, sdp_large_eig.hip ask here and
// decide nothing themselves; plain C++17, no HIP: the rules are tested on the CPU by tests/sdp_large_forms/forms_table.cpp against
// their Python restatement in tests/_sdp_large_forms.py).  Rules only: what a form costs and why it won is written at its kernel.
#pragma once
#include <stddef.h>

// The padded order of a handle's large cones, from the order of the largest: every matrix of the workspace has it.
inline int lg_padded_order(int r_max) { return r_max <= 256 ? 256 : (r_max <= 512 ? 512 : (r_max <= 1024 ? 1024 : 2048)); }

// The block one-sided Jacobi of a padded order: k_lg_jacobi<threads, epl> on column blocks `block` wide.  A column pair has
// threads / block lanes of epl elements each (rp == epl * threads / block); rp / block blocks, half as many workgroups.
enum LgJacobiKernel { LG_JACOBI_256_8, LG_JACOBI_1024_8, LG_JACOBI_512_16, LG_JACOBI_256_32 };
struct LgJacobiForm { LgJacobiKernel kernel; int threads, epl, block; };
inline LgJacobiForm lg_jacobi_form(int rp) {
    if (rp <= 256) return {LG_JACOBI_256_8, 256, 8, 8};
    if (rp <= 512) return {LG_JACOBI_1024_8, 1024, 8, 16};
    if (rp <= 1024) return {LG_JACOBI_512_16, 512, 16, 8};
    return {LG_JACOBI_256_32, 256, 32, 4};              // two blocks of 4 columns are a CU's LDS
}

// A single product C = A B' over all tiles runs on the 16x16 split-k tile (k_gemm_nt_small), not on the 64x64 one.  The same
// predicate lets apply and the max-step read mat(x) from, and write vecm to, the vector itself (the tile's BVEC / CVEC forms).
inline bool lg_small_product(int rp) { return rp <= 256; }

// The v- and s-side max-steps of a pair can run side by side: only the Lanczos form has per-side words and vectors.
inline bool lg_pairable(int rp, int lanczos_mode) { return rp <= 256 && lanczos_mode != 0; }

// The extreme eigenvalue of the max-step's matrix of order r under Lanczos mode 0 .. 3 (cip_set_sdp_lanczos).
enum LgEigKind {
    LG_EIG_LANCZOS,          // k_lg_lanczos1: one workgroup, the matrix in registers; modes 2 and 3 add the inertia certificate
    LG_EIG_REGISTERS,        // k_lg_tridiag1: one workgroup, the matrix in registers, then Sturm
    LG_EIG_COOPERATIVE,      // k_lg_tridiag: a slab of columns in the LDS of each of nwg workgroups, then Sturm
    LG_EIG_STEPPED           // k_tg_*: the matrix in global memory, `launches` launches, then Sturm
};
struct LgEigForm {
    LgEigKind kind;
    bool certificate;        // Lanczos: the inertia certificate follows
    int slab, nwg;           // cooperative: columns per workgroup, workgroups
    size_t lds;              // cooperative: dynamic LDS bytes of a workgroup
    int launches;            // stepped: k_tg_init + (r - 1) k_tg_symv + (r - 2) k_tg_rank2
};
// a slab (pitch r | 1), three r-vectors and 64 doubles of reduction scratch
inline size_t lg_slab_lds(int slab, int r) { return ((size_t)slab * (r | 1) + 3 * (size_t)r + 64) * sizeof(double); }
inline LgEigForm lg_eig_form(int r, int lanczos_mode) {
    LgEigForm f{LG_EIG_REGISTERS, false, 0, 0, 0, 0};
    if (r <= 256) {
        if (lanczos_mode) { f.kind = LG_EIG_LANCZOS; f.certificate = lanczos_mode >= 2; }
    } else if (r <= 1024) {
        // a workgroup keeps 32 columns for the whole reduction; above order 583 that no longer fits 160 KiB: 16 columns
        f.kind = LG_EIG_COOPERATIVE;
        f.slab = lg_slab_lds(32, r) <= 160 * 1024 ? 32 : 16;
        f.nwg = (r + f.slab - 1) / f.slab;
        f.lds = lg_slab_lds(f.slab, r);
    } else {
        f.kind = LG_EIG_STEPPED;
        f.launches = 2 * (r - 1);
    }
    return f;
}
