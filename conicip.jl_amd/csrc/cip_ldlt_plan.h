// The schedule of ONE LDL' factorisation, decided once before its first launch (ldlt.hip walks it; plain C++17, no HIP: the
// rules are tested on the CPU by tests/ldlt_plan/plan_table.cpp against their Python restatement in tests/_ldlt_ref.py).
//
// Inputs: the process-wide settings as they stood when the factorisation began (LdltKnobs, snapshot in ldlt.hip: ldlt_knobs)
// and what the caller is (LdltCtx).  The plan fixes, for the length of the factorisation, every outer block's width, which
// panel chain runs and where the solve preparation forks to the side stream: a setter on another thread changes the NEXT
// factorisation, never the blocks or panels of this one.  The widths are a function of the order and the column only -- not of
// the batch: lock-step groups reproduce the one-problem loop bit for bit.
#pragma once

struct LdltKnobs {
    int nbo;                  // the set outer block (cip_set_ldlt_outer_block); 0: automatic
    int nbo_auto;             // automatic width from order 4096 on with the one-launch chain (CIP_LDLT_NBO_AUTO, 896)
    int tail;                 // the last block takes everything once no more than this is left (CIP_LDLT_TAIL, 2816)
    int chain;                // 3: one launch per panel, 0: three (cip_set_ldlt_fused_chain)
    // solve preparation beside the last block's panel chain (cip_set_ldlt_side_prep), from this many columns before the end on
    // (CIP_SIDE_PREP_FROM, 2048)
    int side_prep, side_from;
    // lock-step groups run the one-launch chain up to this many problems (CIP_LOCKSTEP_PANEL_MAX, 32) and while their long-lived
    // workgroups are no more than this (4 x CUs, CIP_LOCKSTEP_PANEL_CUS)
    int ls_panel_max, ls_panel_cus;
};
struct LdltCtx {
    int Npad, Bs;             // order (a multiple of 128) and the workspace's solve block
    int B;                    // problems of the calling thread's lock-step batch (1: not in a batch)
    bool recording;           // the launches are recorded into a graph
    bool has_side;            // the workspace's owner keeps a side stream
    bool unfused;             // the workspace gave up on the one-launch chain
};

// width rule without the wide last block: the set value, else the automatic one
inline int ldlt_outer_block(const LdltKnobs &k, int Npad) { return k.nbo > 0 ? k.nbo : (Npad >= 4096 && k.chain) ? k.nbo_auto : 512; }

struct LdltPlan {
    int Npad, Bs;
    int nbo;                  // every block but a wide last one
    int tail;                 // the block that starts with at most `tail` columns left takes them all (0: no such block)
    bool fused;               // the one-launch panel chain (the give-up hook's and a recorded graph's "ran fused")
    int fork_C0;              // first column of the last block when its panels fork solve preparation, else -1
    int fork_step, side_from; // forks at multiples of fork_step, no earlier than side_from columns before the end

    int width_at(int C0) const { const int left = Npad - C0; return (left <= tail || left < nbo) ? left : nbo; }
    // The side-stream group that forks when the panel chain stands at column c with the solve blocks [0, Jdone) taken: it
    // takes [Jdone, J1), J1 returned; 0: no fork here.  c: a solve-block boundary inside the last block (or its start), or
    // Npad -- the last group, forked behind the last panel, if anything forked before.
    int next_fork(int c, int Jdone) const {
        if (fork_C0 < 0) return 0;
        if (c >= Npad) return Jdone > 0 ? Npad / Bs : 0;
        return (c % fork_step == 0 && Npad - c <= side_from && c / Bs > Jdone) ? c / Bs : 0;
    }
};

inline LdltPlan ldlt_plan(const LdltKnobs &k, const LdltCtx &x) {
    LdltPlan p{};
    p.Npad = x.Npad; p.Bs = x.Bs; p.nbo = ldlt_outer_block(k, x.Npad);
    p.tail = (k.nbo == 0 && p.nbo >= 640 && k.tail > 0) ? k.tail : 0;       // automatic widths only
    // the one-launch chain when it has the chip to itself, and in lock-step groups while the group's long-lived workgroups
    // (10 + Npad / 64 per problem at the first panel) are no more than about four rounds of the chip (ldlt.hip)
    const bool small_group = x.B <= k.ls_panel_max && (long)x.B * (10 + x.Npad / 64) <= k.ls_panel_cus;
    p.fused = x.Npad > 0 && k.chain && !x.unfused && (x.B <= 1 || small_group);
    // side preparation only in a wide last block -- at least two regular widths, wider than the solve block -- of a matrix
    // with more than one solve block; never in batches or recordings
    int C0 = 0;                                          // ... where the last block starts
    while (C0 + p.width_at(C0) < x.Npad) C0 += p.width_at(C0);
    const int wlast = x.Npad - C0;
    const bool forks = k.side_prep && x.B <= 1 && !x.recording && x.has_side && x.Bs > 128 && x.Npad / x.Bs >= 2 &&
                       wlast >= 2 * p.nbo && wlast > x.Bs;
    p.fork_C0 = forks ? C0 : -1; p.side_from = k.side_from;
    p.fork_step = x.Bs > 1024 ? x.Bs : 1024;            // no finer than 1024 columns (a fork per 512-wide solve block lost)
    return p;
}
