"""The dispatch rules of the large S cones (conicip.jl_amd/csrc/cip_sdp_large_forms.h), restated in Python: which padded order,
Jacobi form, GEMM kernel and max-step eigenvalue form a set of cones reaches.  tests/test_gpu_sdp_large_edges.py holds its case
table against it; tests/test_sdp_large_forms.py holds it against the header itself, order by order."""
import _cone_ref as CR

LARGE_S_MIN = 133                   # sdp.hip below, the chip-wide path (sdp_large*.hip) from here
# what each case of tests/test_gpu_sdp_large_edges.py (CASES) is there to reach, at the default Lanczos mode
PATHS = {
    "s257": {"rp": 512, "jacobi": (1024, 8, 16), "gemm": "batched-64", "pairable": False, "maxstep": [("cooperative", 32, 9)]},
    "s512": {"rp": 512, "jacobi": (1024, 8, 16), "gemm": "batched-64", "pairable": False, "maxstep": [("cooperative", 32, 16)]},
    "s513": {"rp": 1024, "jacobi": (512, 16, 8), "gemm": "batched-64", "pairable": False, "maxstep": [("cooperative", 32, 17)]},
    "s583": {"rp": 1024, "jacobi": (512, 16, 8), "gemm": "batched-64", "pairable": False, "maxstep": [("cooperative", 32, 19)]},
    "s584": {"rp": 1024, "jacobi": (512, 16, 8), "gemm": "batched-64", "pairable": False, "maxstep": [("cooperative", 16, 37)]},
    "s1024": {"rp": 1024, "jacobi": (512, 16, 8), "gemm": "batched-64", "pairable": False, "maxstep": [("cooperative", 16, 64)]},
    "s1025": {"rp": 2048, "jacobi": (256, 32, 4), "gemm": "batched-64", "pairable": False, "maxstep": [("stepped", 0, 2 * 1024)]},
    "mixed_140_300": {"rp": 512, "jacobi": (1024, 8, 16), "gemm": "batched-64", "pairable": False,
                      "maxstep": [("lanczos", 0, 1), ("cooperative", 32, 10)], "padding": [372, 212]},
}


def _reach(cone_dims, mode=2):
    """the dispatch rules of cip_sdp_large_forms.h: the padded order from the largest large cone (lg_padded_order); per rp the
    Jacobi form (threads, elements per lane, block width: lg_jacobi_form); k_gemm_nt_small at rp <= 256 only (lg_small_product),
    the paired max step there and under a Lanczos mode only (lg_pairable); the max step's eigenvalue (lg_eig_form) up to order 256
    by Lanczos, in mode 0 by the register tridiagonalisation; by the cooperative tridiagonalisation up to 1024 (slabs of 32
    columns while (slab (r | 1) + 3 r + 64) doubles fit 160 KiB, else 16; one workgroup per slab); 2 (r - 1) stepped launches
    above.  maxstep: (form, slab, workgroups or launches) per large cone"""
    large = [CR.order(k) for t, k in cone_dims if t == "S" and CR.order(k) >= LARGE_S_MIN]
    rmax = max(large)
    rp = 256 if rmax <= 256 else 512 if rmax <= 512 else 1024 if rmax <= 1024 else 2048
    out = {"rp": rp, "gemm": "small" if rp <= 256 else "batched-64", "pairable": rp <= 256 and mode != 0,
           "jacobi": {256: (256, 8, 8), 512: (1024, 8, 16), 1024: (512, 16, 8), 2048: (256, 32, 4)}[rp],
           "padding": [rp - r for r in large], "maxstep": []}
    for r in large:
        if r > 1024:
            out["maxstep"].append(("stepped", 0, 2 * (r - 1)))
        elif r <= 256:
            out["maxstep"].append(("lanczos", 0, 1) if mode else ("registers", 0, 1))
        else:
            slab = 32 if (32 * (r | 1) + 3 * r + 64) * 8 <= 160 * 1024 else 16
            out["maxstep"].append(("cooperative", slab, -(-r // slab)))
    return out
