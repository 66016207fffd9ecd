// sqp_group_body.inc -- the body of the 16-lane kernels (kernel text, not a header: sqp_group.h includes it inside each
// of its three __global__ templates, behind their constexpr flags).  This file is the spine: instance setup, the
// iteration loop, the write-back.  The phases are included from here, each once and in program order:
//   sqp_group_phase_a.inc        A: stage evaluation, barrier terms, reductions
//   sqp_group_serial.inc         the one-lane sweeps of the models with nx + nu >= 16 (called from the two !DIST branches)
//   sqp_group_dist_grad.inc      lane-distributed: d recursion, adjoint, gradient, the loads of A_k's rows and columns
//   sqp_group_dist_riccati.inc   lane-distributed: Riccati sweep, and its vector part for Mehrotra's corrector
//   sqp_group_wpass.inc          the exact-Hessian W pass
//   sqp_group_step.inc           lane-distributed: step sweep, QP passes, predictor-corrector block, dJ
//   sqp_group_linesearch.inc     D: step limits, line search, update
// expects: Model, BOUNDED, XB, EXACT, MEHR, IB (constexpr), p (SolveParams), gw (GroupWork).
    static_assert(!(BOUNDED && XB), "the interior-point variant handles the control bounds itself");
    static_assert(!MEHR || XB, "the barrier rule belongs to the interior-point variant");
    constexpr int NX = Model::NX, NU = Model::NU, NQ = Model::NQ, NA = NX - NQ, NS = NX + NU;
    constexpr int SQ = NA * NQ > 0 ? NA * NQ : 1;  // extent of the h da/dq block (empty for NQ = 0)
    constexpr int FQ = NA * NQ, FD = NA * NA, FU = NA * NU;  // stage block sizes (sqp_lane.h a_mul)
    static_assert(NQ >= 0 && NA >= NQ, "x = [q; z] with qdot = z[0:NQ]");
    constexpr int G = kGroupLanes;
    extern __shared__ double shm[];
    const int gl = threadIdx.x & (G - 1);
    const int gi = threadIdx.x / G;
    [[maybe_unused]] const int lane0 = threadIdx.x;
    MMPC_PHASE_DECL
    const int gbase = gi * G;  // first lane of this instance's group
    // slot of this group in the launch: the instance itself, or (resume launch, p.tail_idx) an entry of the lane
    // kernel's hand-over list
    const int64_t slot = (int64_t)blockIdx.x * p.gpw + gi;
    const bool resume = p.tail_idx != nullptr;
    const bool valid = gi < p.gpw && slot < (resume ? (int64_t)min(*p.tail_count, p.tail_slots) : p.B);
    // a group past the end of the batch (the last wave of a B not divisible by 4) leaves at once: no group reads
    // another group's lanes (row_bcast and the group reductions stay inside the 16-lane row) or LDS block, so
    // nothing else in the wave needs it, and it issues no memory access at all (round 4 had those groups run on
    // aliased to instance 0 and masked by `done`, which made every store's masking a correctness condition)
    if (!valid) return;
    const int64_t inst = resume ? (int64_t)p.tail_idx[slot] : slot;
    const int N = p.N;
    const int NV = NX * (N + 1) + NU * N;
    const double h = p.h;

    // ---- LDS views of this instance: the layout of group_lds (sqp_group.h), as a pointer chain (group_lds_chain_ok) ----
    // constant block of the per-lane sweep operands (LOPS, below): the models with GroupLaneOps, lane-distributed path
    constexpr int KC = NX + NU < kGroupLanes ? GroupLaneOps<Model>::doubles : 0;
    // head block of the gain record (group_lds): the unbounded kernels of those models
    constexpr int KH = (KC > 0 && !BOUNDED && !XB) ? group_head_doubles(NX, NU) : 0;
    double* const sX = shm + gi * group_lds_doubles(NX, NU, NQ, N, BOUNDED, p.is_linear != 0, KC, KH);  // [N+1][NX]
    // sD | sDX | sDU are contiguous: between the W pass and the step sweep of an iteration all three are dead (d / lam
    // in sD: the W pass is its last reader; sDX, sDU: the previous step, consumed by the update) and, on the on-chip W
    // path (WLDS), sD + NX .. holds the packed W records (sW) -- d_0 = 0 in sD[0..NX) stays
    double* const sU = sX + (N + 1) * NX;                          // [N][NU]
    double* const sD = sU + N * NU;                                // [N+1][NX]
    double* const sDX = sD + (N + 1) * NX;                         // [N+1][NX]
    double* const sDU = sDX + (N + 1) * NX;                        // [N][NU]
    double* const sF = sDU + N * NU;                               // [N][NX]
    double* const sC = sF + N * NX;                                // [N][NX]
    double* const sFq = sC + N * NX;                               // [N][NA*NQ]   h da/dq
    double* const sFqd = sFq + N * FQ;                             // [N][NA*NA]   h da/dz
    double* const sFu = sFqd + N * FD;                             // [N][NA*NU]   h da/du
    double* const sR = sFu + N * FU;                               // [N][NX]      targets r_k
    double* const sHold = sR + N * NX;                             // [N][NU]      bound a control is held at
    double* const sLin = sHold + (BOUNDED ? N * NU : 0);           // linear mode: Fq | Fqd | Fu | xdot
    // On-chip W path: the unbounded exact-Hessian solve of a control-affine model with a packed W record that fits the
    // dead arrays (PK <= 2 NX + NU per stage; PK >= NX for the W pass's write order, below).  It solves the QP once per
    // iteration, with no step sweep between the W pass and the Riccati sweep; the control-bounded and interior-point
    // variants solve it again after step sweeps that rewrite sDX, sD and sDU, and keep W in the workspace.
    constexpr int PK = WPack<Model>::PK;
    constexpr bool WLDS = EXACT && !BOUNDED && !XB && IsControlAffine<Model>::value && PK >= NX && PK <= 2 * NX + NU;
    double* const wK = gw.ws + slot * (int64_t)group_ws_doubles(NX, NU, N, BOUNDED, XB, WLDS, MEHR);  // [N][NU][NS+1]
    constexpr int HW = group_hess_doubles(NX, NU);
    double* const wH = wK + N * NU * (NS + 1);  // EXACT: [N][HW] = W_k x rows [NX][NS] | W_k uu block [NU][NU]
    double* const sW = sD + NX;                 // WLDS: [N][PK] packed W_k x rows, over sD[1..], sDX and sDU
    // WLDS: the sweep's loads of the last record's structural zeros reach the OVER doubles behind it (WPack).  Those
    // lie inside sDX | sDU (OVER <= NX and PK <= 2 NX + NU): zeroed here for the first iteration, and from then on a
    // step of the previous iteration, finite whenever the iteration goes on to its Riccati sweep -- the line search
    // accepts a non-finite step only into an iterate that the next stop test leaves with ST_NONFINITE.
    static_assert(!WLDS || WPack<Model>::OVER <= NX, "the over-read of the last W record stays inside sDU");
    if constexpr (WLDS) {
        if (gl < WPack<Model>::OVER) sW[N * PK + gl] = 0.0;
    }
    constexpr int NR = NS + NU + 1;             // BOUNDED: [N][NU][NR] = un-held [H_wx | -R | H_ww | h_w] rows
    double* const wRel = wH + N * HW;
    bool w_zeros_stored = false;   // W_k's structural zeros are in the workspace (this launch's first W pass stored them)
    // interior point (XB): per stage k, y = (x_{k+1} | u_k) [NS]: duals z_l, z_u, Sigma, b, z_u - z_l -- in the HBM
    // workspace after the W blocks (group_ws_doubles); the stage-parallel phases write them, the serial sweeps read
    // them on other lanes after a workgroup fence
    double* const sZl = wRel;  // [N][NS]
    double* const sZu = sZl + N * NS;
    double* const sSg = sZu + N * NS;
    double* const sBb = sSg + N * NS;
    double* const sZg = sBb + N * NS;
    // MEHR: corrector terms mu_t - ds_aff dz_aff of the lower / upper bounds, written and read by the stage's own lane
    [[maybe_unused]] double* const sCl = sZg + N * NS;   // [N][NS]
    [[maybe_unused]] double* const sCu = sCl + N * NS;
    // MEHR: what the predictor's Riccati sweep (backward_dist) leaves per stage for the corrector's vector-only sweep
    // (backward_vec).  Per lane r [VL][G]: pc = P~_{k+1,x} row r . c_k, pn0 = the b-independent part of row r of p~_k,
    // Ytil[NU] = column r of L^-1 [H_wx | -R]; once [VS]: L row by row with 1 / L_aa on the diagonal, then the
    // b-independent part of h_w (bit-identical on every lane: each lane stores and reads them)
    constexpr int VL = 2 + NU, VC = NU * (NU + 1) / 2, VS = VC + NU, VR = VL * G + VS;
    [[maybe_unused]] double* const sVr = sCu + N * NS;   // [N][VR]
    const double* const trg = p.traj + inst * (int64_t)N * NX;

    // two stages per lane in the stage-parallel phases (PAIR, below): the width of phase A, of the fused trial, of the W
    // pass, of the prologue and of the update
    constexpr bool PAIR = HasWideEval<Model>::value && !BOUNDED && !XB;
    constexpr int WD = PAIR ? 2 : 1;
    const double* w = p.weights + inst * p.w_stride;
    double Q[NX], R[NU], Rm[NU], up[NU];
#pragma unroll
    for (int r = 0; r < NX; ++r) Q[r] = w[r];
#pragma unroll
    for (int c = 0; c < NU; ++c) {
        R[c] = w[NX + c];
        Rm[c] = w[NX + NU + c];
        up[c] = p.u_prev[inst * NU + c];
    }
    double lbv[NU], ubv[NU];
    load_bounds<NU, BOUNDED, IB>(p, inst, lbv, ubv);
    // PAIR: the prologue in one round trip.  Every global load of the lane is issued here, behind the weights and u_prev
    // and before anything waits for one of them: x_0, and for the lane's first pair of stages (gl and gl + G: the whole
    // horizon up to N = 2 G - 1) the targets and, unless the start is zero, V.  The LDS stores and the per-lane
    // constants derived from the weights follow.  The uniform init_zero test is taken once, around the loads; a stage
    // index past the horizon is clamped (k to the lane's first stage, the u / target row of k = N to N - 1), so the
    // loads need no lane test and a repeated store writes the value already there.
    [[maybe_unused]] double px0[NX], pxv[WD][NX], puv[WD][NU], prv[WD][NX];
    // (a lane past the end of a short horizon, gl > N, loads stage N's values and stores nothing)
    [[maybe_unused]] auto pro_k = [&](int k0, int e) { return k0 + e * G <= N ? k0 + e * G : (k0 <= N ? k0 : N); };
    [[maybe_unused]] auto pro_load = [&](int k0, double (*xv)[NX], double (*uv)[NU], double (*rv)[NX]) {
        const double* Vin = p.V + inst * (int64_t)NV;
#pragma unroll
        for (int e = 0; e < WD; ++e) {
            const int k = pro_k(k0, e), ku = k < N ? k : N - 1;
#pragma unroll
            for (int r = 0; r < NX; ++r) rv[e][r] = trg[ku * NX + r];
        }
        if (p.init_zero) {
#pragma unroll
            for (int e = 0; e < WD; ++e) {
#pragma unroll
                for (int r = 0; r < NX; ++r) xv[e][r] = 0.0;
#pragma unroll
                for (int c = 0; c < NU; ++c) uv[e][c] = 0.0;
            }
        } else {
#pragma unroll
            for (int e = 0; e < WD; ++e) {
                const int k = pro_k(k0, e), ku = k < N ? k : N - 1;
#pragma unroll
                for (int r = 0; r < NX; ++r) xv[e][r] = Vin[k * NS + r];
#pragma unroll
                for (int c = 0; c < NU; ++c) uv[e][c] = Vin[ku * NS + NX + c];
            }
        }
    };
    if constexpr (PAIR) {
#pragma unroll
        for (int r = 0; r < NX; ++r) px0[r] = p.x0[inst * NX + r];
        pro_load(gl, pxv, puv, prv);
    }
    // ---- lane-distributed Riccati (DIST): lane r of the group owns row r of the augmented value function
    //      P~ (NS x NS) and of every per-row quantity; small per-stage quantities are computed redundantly on
    //      all lanes; rows are exchanged with row_bcast (DESIGN.md 4c).  Control bounds (BOUNDED) run the same
    //      sweeps with the held controls of the projected SQP folded into the per-stage quantities; state bounds
    //      (XB) add the barrier terms and use the Cholesky (Y^T Y) form of the stage update.  Models with
    //      nx + nu >= 16 keep the one-lane sweep below. ----
    constexpr bool DIST = (NS < G);
    static_assert(!MEHR || DIST, "Mehrotra's rule: lane-distributed path");
    // control-affine model: the u-u block of the exact-Hessian W_k is zero -- neither stored, loaded nor added
    constexpr bool CAFF = IsControlAffine<Model>::value;
    static_assert(!EXACT || (DIST && HasHess<Model>::value), "exact Hessian: lane-distributed path, model eval_hess");
    const int r = gl;
    const bool lx = r < NX, lu = r >= NX && r < NS, la = r >= NQ && r < NX;
    const int rx = lx ? r : 0;                        // x row of this lane (clamped for address arithmetic)
    const int ru = lu ? r - NX : 0;                   // u row
    const int ta = la ? r - NQ : 0;                   // row of the a-blocks (hFq, hFqd, hFu) of an a-lane
    const double Qr = lx ? w[rx] : 0.0;               // Q of this lane's x row
    // lane-role masks as blend factors, for the models whose row / column of A is not a per-lane load (LOPS, ACOLP,
    // below): their DIST loops blend loaded values with FMAs instead of selects (a select of an LDS load becomes a
    // branch or a pointer select)
    [[maybe_unused]] const double lqd = r < NQ ? 1.0 : 0.0, lad = la ? 1.0 : 0.0;
    // x-lane factor for the sweeps' per-stage masking: one FP64 multiply where a 64-bit select is two cndmasks (the
    // masked values are finite sums of this instance's own data, so 0 * v == 0)
    const double lxf = lx ? 1.0 : 0.0;
    // WLDS: W_k[r][j] sits at slot wrow + col(j) of the packed record, wrow = col(r) this lane's one row offset (a lane
    // without an x row: row 0), and wm[j] is its blend factor.  A structural zero, and every column of a lane without
    // an x row, reads its additive slot all the same -- another entry of this record, or up to OVER doubles past it, all
    // finite (sW, below) -- under a factor 0; the factor takes the place of the x-lane factor at the uses of W, so the
    // sweep gains no select; columns with the same zero pattern share one factor.
    int wrow = 0;
#pragma unroll
    for (int r2 = 0; r2 < NX; ++r2)
        if (lx && r == r2) wrow = WPack<Model>::col(r2);
    double wm[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        bool nz = false;
#pragma unroll
        for (int r2 = 0; r2 < NX; ++r2)
            if (lx && r == r2 && WPack<Model>::idx(r2, j) >= 0) nz = true;
        wm[j] = wpack_col_rep<Model>(j) < j ? wm[wpack_col_rep<Model>(j)] : (nz ? 1.0 : 0.0);
    }
    const int rq = r < NQ ? r : 0;                    // q column of a q-lane (clamped)
    const double Rr = lu ? w[NX + ru] : 0.0;          // R of this lane's u row
    double dgx[NS];                                    // XB: this x-lane's diagonal entry of P~ (barrier Sigma)
#pragma unroll
    for (int j = 0; j < NS; ++j) dgx[j] = (lx && j == r) ? 1.0 : 0.0;
    double lbr = -INFINITY, ubr = INFINITY;            // bounds of this u-lane's control (BOUNDED)
#pragma unroll
    for (int c = 0; c < NU; ++c)
        if (lu && ru == c) {
            lbr = lbv[c];
            ubr = ubv[c];
        }
    double hq[NQ > 0 ? NQ : 1], hrow[NX], qoh[NX], rdg[NU];
#pragma unroll
    for (int z = 0; z < NQ; ++z) hq[z] = (r == NQ + z) ? h : 0.0;   // column r of A holds h in row z (kinematics)
#pragma unroll
    for (int j = 0; j < NX; ++j) {
        hrow[j] = (r < NQ && j == NQ + r) ? h : 0.0;  // row r of A of a q-lane (besides the identity); blended where !LOPS
        qoh[j] = (j == r) ? Qr : 0.0;
    }
#pragma unroll
    for (int c = 0; c < NU; ++c) rdg[c] = (r == NX + c) ? R[c] : 0.0;
    // LOPS (models with GroupLaneOps): this lane's row and column of A_k as LDS operands of the serial sweeps -- an address and a stage stride
    // (bytes) per operand, both fixed for the launch.  A lane with the role reads the stage blocks (stride = block size);
    // a q-lane's row h e_{NQ+r} and the zero row / column of a lane without the role are read from the constant block
    // sKc = [NX - 1 zeros | h | max(NX, NU) zeros] with stride 0.  The loads are unconditional and deliver what the
    // blends fma(lad, v, hrow) / lad v + lqd v' delivered (1 v + 0, or 0 v + h with v finite), without the FP64
    // instructions -- the same idiom as the W slots (wrow): per-lane addresses, never a select of a loaded value.
    constexpr bool LOPS = KC > 0;
    double* const sKc = sX + group_lds_doubles(NX, NU, NQ, N, BOUNDED, p.is_linear != 0, KC, KH) - KC;
    [[maybe_unused]] double* const sKh = sKc - KH;   // [3][NU][NS+1]: K_k | kff_k of stages 0 .. 2
    // (the addresses are LDS pointers, so that the base of the dynamic LDS is added here once and not at every load)
    using LdsB = const __attribute__((address_space(3))) char*;
    using LdsD = const __attribute__((address_space(3))) double*;
    const LdsB shb = (LdsB)shm;
    auto lds = [](LdsB b) { return *(LdsD)b; };
    // a running address, opaque to the loop optimiser: one add per stage and immediate offsets from it (left alone,
    // strength reduction gives every unrolled copy of a load its own induction variable)
    auto pin = [](LdsB& b) { asm volatile("" : "+v"(b)); };
    [[maybe_unused]] const LdsB iKc = shb + 8 * (int)(sKc - shm), iKz = iKc + 8 * NX;   // the block; its zero row (max(NX, NU) zeros)
    // row r of [A - I | B]: a-lanes [hFq | hFqd | hFu] row r - NQ, q-lanes h e_{NQ+r} | 0.
    // MIRROR: a lane without an x row takes row 0's operands (rx = 0: the addresses of lane 0, a q-lane) in the d
    // recursion, the adjoint and the step sweep, so it carries lane 0's chain bit for bit (same instructions, same
    // operands, same broadcasts) and the sweeps store without a lane mask: its stores go to lane 0's address with lane
    // 0's value.  It never reaches another group: every address is this instance's own.  (The u-lanes of the step sweep
    // keep their own chain; see there.)  Without MIRROR such a lane reads the zero row and its stores stay masked.
    constexpr bool MIRROR = LOPS && NQ > 0 && NQ == NA && (NA - 1) * NA < KC;   // (= ACOLP, below)
    [[maybe_unused]] const double Qa = MIRROR ? w[rx] : Qr;   // Q of the x row whose chain the lane carries in the adjoint
    [[maybe_unused]] const LdsB iAq =
        la ? shb + 8 * ((int)(sFq - shm) + ta * NQ) : ((r < NQ || MIRROR) ? iKc + 8 * ((NX - 1) - (NQ + rq)) : iKz);
    [[maybe_unused]] const int zAq = la ? 8 * FQ : 0, zAd = la ? 8 * FD : 0, zBr = la ? 8 * FU : 0;
    [[maybe_unused]] const LdsB iAd = la ? shb + 8 * ((int)(sFqd - shm) + ta * NA) : ((r < NQ || MIRROR) ? iAq + 8 * NQ : iKz);
    [[maybe_unused]] const LdsB iBr = la ? shb + 8 * ((int)(sFu - shm) + ta * NU) : iKz;
    // column r of A's a-rows: a-lanes hFqd[:, r - NQ], q-lanes hFq[:, r], other lanes 0.  With NQ == NA both kinds of
    // column have the element stride NA, an immediate; a lane without the role reads the block from its start, where
    // the offsets t NA (t < NA) are zeros (they never meet h at NX - 1 = 2 NA - 1).  Other shapes keep the blend.
    constexpr bool ACOLP = LOPS && NQ == NA && (NA - 1) * NA < KC;
    static_assert(!MIRROR || ACOLP, "a mirrored lane reads row 0's column through the per-lane column address");
    [[maybe_unused]] const int zAc = (la || r < NQ) ? 8 * FD : 0;
    [[maybe_unused]] const LdsB iAc = la ? shb + 8 * ((int)(sFqd - shm) + ta) : (r < NQ ? shb + 8 * ((int)(sFq - shm) + rq) : iKc),
                                iAcN = iAc + (N - 1) * zAc;   // ... at the last stage
    if constexpr (LOPS) {
        for (int i = gl; i < KC; i += G) sKc[i] = (i == NX - 1) ? h : 0.0;
    }
    // ---- load: V (reference layout) -> LDS, x_0 pinned (ModelControl.cpp:144-145) ----
    if constexpr (PAIR) {
        // the first pair's values are in flight since the top (pro_load); a horizon of more than two rounds loads its
        // further pairs here, one round trip each
        const bool hold = p.init_hold != 0;
        for (int k0 = gl; k0 <= N; k0 += WD * G) {
            if (k0 != gl) pro_load(k0, pxv, puv, prv);
#pragma unroll
            for (int e = 0; e < WD; ++e) {
                const int k = pro_k(k0, e), ku = k < N ? k : N - 1;
#pragma unroll
                for (int r = 0; r < NX; ++r) sX[k * NX + r] = (k == 0 || hold) ? px0[r] : pxv[e][r];
#pragma unroll
                for (int c = 0; c < NU; ++c) sU[ku * NU + c] = puv[e][c];
#pragma unroll
                for (int r = 0; r < NX; ++r) sR[ku * NX + r] = prv[e][r];
            }
        }
    } else {
        const double* Vin = p.V + inst * (int64_t)NV;
        for (int k = gl; k <= N; k += G) {
#pragma unroll
            for (int r = 0; r < NX; ++r)
                sX[k * NX + r] = (k == 0 || p.init_hold) ? p.x0[inst * NX + r] : (p.init_zero ? 0.0 : Vin[k * NS + r]);
            if (k < N) {
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    const double v = p.init_zero ? 0.0 : Vin[k * NS + NX + c];
                    sU[k * NU + c] = BOUNDED ? proj(v, lbv[c], ubv[c]) : v;
                }
#pragma unroll
                for (int r = 0; r < NX; ++r) sR[k * NX + r] = trg[k * NX + r];
            }
        }
    }
    const double* const tr = sR;   // the targets as the phases read them (reading sR itself changes the cfg#2 kernels' code)
    double yl[XB ? NS : 1], yu[XB ? NS : 1];
    double mub = (XB && resume) ? p.tail_mub[slot] : kIpMu0;  // barrier parameter (f = J/2 scale)
    if constexpr (XB) {
        load_ip_bounds<NX, NU, IB>(p, inst, yl, yu);
        __builtin_amdgcn_wave_barrier();
        if (resume) {   // the handed-over duals, from the lane launch's workspace (the iterate is interior already)
            const double* const lz = p.tail_lws + (inst >> 6) * p.tail_lws_block + (inst & 63);
            for (int k = gl; k < N; k += G) {
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    sZl[k * NS + j] = lz[((int64_t)k * p.tail_lws_ss + p.tail_lws_zl + j) * 64];
                    sZu[k * NS + j] = lz[((int64_t)k * p.tail_lws_ss + p.tail_lws_zl + NS + j) * 64];
                }
            }
        } else {
            // y pushed into the interior, z = 1 on finite bounds (oracle solve_one_ip)
            for (int k = gl; k < N; k += G) {
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    double& y = j < NX ? sX[(k + 1) * NX + j] : sU[k * NU + j - NX];
                    y = ip_push(y, yl[j], yu[j]);
                    sZl[k * NS + j] = yl[j] > -INFINITY ? 1.0 : 0.0;
                    sZu[k * NS + j] = yu[j] < INFINITY ? 1.0 : 0.0;
                }
            }
        }
    }
    // linear mode: acceleration Jacobians and xdot at (x_0, u_prev) (ModelControl.cpp:125-135), in LDS (keeps
    // 20-64 VGPRs free for the serial Riccati sweep); the linearisation point x_0 is sX[0..NX) (pinned)
    const bool lin = p.is_linear != 0;
    double* const lFq = sLin;
    double* const lFqd = lFq + FQ;
    double* const lFu = lFqd + FD;
    double* const lxd = lFu + FU;
    const double* const lxs = sX;
    if (lin && gl == 0) {
        double acc[NA], x[NX], Fq[SQ], Fqd[FD], Fu[FU];
#pragma unroll
        for (int r = 0; r < NX; ++r) x[r] = p.x0[inst * NX + r];
        Model::eval_acc_jac(x, up, acc, Fq, Fqd, Fu);
#pragma unroll
        for (int i = 0; i < FQ; ++i) lFq[i] = Fq[i];
#pragma unroll
        for (int i = 0; i < FD; ++i) lFqd[i] = Fqd[i];
#pragma unroll
        for (int i = 0; i < FU; ++i) lFu[i] = Fu[i];
#pragma unroll
        for (int i = 0; i < NQ; ++i) lxd[i] = x[NQ + i];
#pragma unroll
        for (int i = 0; i < NA; ++i) lxd[NQ + i] = acc[i];
    }
    __builtin_amdgcn_wave_barrier();
    int status = ST_MAX_ITER;
    int it = 0;
    double kkt = 0.0, mu = resume ? p.tail_mu[slot] : 0.0, pg_prev = (BOUNDED && resume) ? p.tail_mub[slot] : INFINITY;
    // PAIR: the stage-parallel phases take TWO stages per lane in one straight-line body, k and k + G (the unbounded
    // solves of a model whose functions take dpack values, HasWideEval: the 2-link arm, cfg#2).  A lane's stage
    // evaluation is one dependent FP64 chain (two range reductions, four Horner polynomials, a division, the quotient
    // rule) that issues every ~8 cycles where the wave could issue every 4; the second stage is an independent chain
    // in the same block, interleaved in the source (group_model_w).  A lane without a second stage (k + G >= N) repeats
    // its own stage k: it stores the same values to the same addresses, the max and non-finite accumulators are
    // idempotent, and the sums (J, |c|_1, dJ) keep their value after the first stage by one select each.  Per stage
    // every operation keeps its operands and order, and every per-lane sum its order (k, then k + G).  For N > 2 G the
    // loops run over pairs of rounds.  WD = 1 (every other kernel) is the one-stage loop as it was.  (PAIR and WD are
    // defined at the prologue, which takes the pairs too.)
    // the stage loops' body with `lin` hoisted (PAIR) or as group_model's run-time argument (LM = -1)
    auto with_lin = [&](auto wd_c, auto&& body) {
        if constexpr (decltype(wd_c)::value == 1) body(std::integral_constant<int, -1>{});
        else if (p.is_linear != 0) body(std::integral_constant<int, 1>{});
        else body(std::integral_constant<int, 0>{});
    };
    bool fwd_ready = false;
    double J0n = 0.0, c1n = 0.0, cmaxn = 0.0;
    int nfn = 0;
    MMPC_PHASE(0);
    for (it = resume ? p.tail_it[slot] : 0;; ++it) {
        MMPC_PHASE(8);
        __builtin_amdgcn_wave_barrier();
#include "sqp_group_phase_a.inc"
        MMPC_PHASE(1);

        // ---- B. one lane: d recursion, then adjoint + gradient + Riccati backward sweep (the 6x6 / 12x12
        //      Riccati step of one stage is too small to pay for lane-parallel exchanges: measured slower) ----
        double gmax = 0.0, lmax = 0.0;
        int fact_ok = 1;
        const double beps = BOUNDED ? fmin(kBoundEps, pg_prev) : 0.0;
#include "sqp_group_serial.inc"
#include "sqp_group_dist_grad.inc"
#include "sqp_group_dist_riccati.inc"
        if constexpr (DIST) {
            d_recursion_dist();
            adjoint_dist();
            lmax = group_max(lmax);
            gmax = group_max(gmax);
        } else if (gl == 0) {   // the serial path (sqp_group_serial.inc): its d recursion, then its first sweep
            {
                double d[NX];
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    d[r] = 0.0;
                    sD[r] = 0.0;
                }
                // the operands of step k+1 are loaded during step k (the recursion is latency-bound)
                double aq[SQ], ad[FD], ac[NX];
#pragma unroll
                for (int i = 0; i < FQ; ++i) aq[i] = sFq[i];
#pragma unroll
                for (int i = 0; i < FD; ++i) ad[i] = sFqd[i];
#pragma unroll
                for (int r = 0; r < NX; ++r) ac[r] = sC[r];
                constexpr int kDUnroll = NX <= 4 ? 2 : 1;
#pragma unroll kDUnroll
                for (int k = 0; k < N; ++k) {
                    double fq[SQ], fd[FD], cc[NX], dn[NX];
#pragma unroll
                    for (int i = 0; i < FQ; ++i) fq[i] = aq[i];
#pragma unroll
                    for (int i = 0; i < FD; ++i) fd[i] = ad[i];
#pragma unroll
                    for (int r = 0; r < NX; ++r) cc[r] = ac[r];
                    const int kn = k + 1 < N ? k + 1 : k;
#pragma unroll
                    for (int i = 0; i < FQ; ++i) aq[i] = sFq[kn * FQ + i];
#pragma unroll
                    for (int i = 0; i < FD; ++i) ad[i] = sFqd[kn * FD + i];
#pragma unroll
                    for (int r = 0; r < NX; ++r) ac[r] = sC[kn * NX + r];
                    a_mul<NQ, NA, double>(h, fq, fd, d, dn);
#pragma unroll
                    for (int r = 0; r < NX; ++r) {
                        d[r] = dn[r] + cc[r];
                        sD[(k + 1) * NX + r] = d[r];
                    }
                }
            }
            backward(0);
        }
        if constexpr (!DIST) {
            gmax = group_bcast(gmax, gbase);
            lmax = group_bcast(lmax, gbase);
            fact_ok = group_bcast_i(fact_ok, gbase);
        }
        MMPC_PHASE(2);
        nonfinite = (group_max((double)nonfinite) != 0.0);
        kkt = fmax(gmax, cmax);
        if (XB) kkt = fmax(kkt, 2.0 * cmpl0);  // J-scale complementarity
        double* trc = p.trace ? p.trace + (inst * (p.max_iter + 1) + it) * 8 : nullptr;
        if (trc && gl == 0) {
            trc[0] = gmax;
            trc[1] = cmax;
            trc[2] = J0;
            trc[3] = c1;
            trc[7] = lmax;
        }
        if (nonfinite || !isfinite(kkt)) {
            status = ST_NONFINITE;
            break;
        }
        if (gmax <= p.tol_grad && cmax <= p.tol_defect && (!XB || 2.0 * cmpl0 <= kIpTolCompl)) {
            status = ST_CONVERGED;
            break;
        }
        if (it == p.max_iter) {
            status = ST_MAX_ITER;
            break;
        }
        MMPC_PHASE(9);
#include "sqp_group_wpass.inc"
        // exact Hessian in this iteration's QP solves (false after a Gauss-Newton fallback)
        bool use_w = EXACT;
        if constexpr (DIST) {   // Riccati sweep (fact_ok is uniform over the group)
            backward_dist(use_w);
            // exact KKT matrix not positive definite on the null space: this iteration takes the Gauss-Newton step
            // (oracle solve_one: Cholesky of the exact condensed Hessian fails -> Gauss-Newton)
            if (EXACT && !fact_ok) {
                fact_ok = 1;
                use_w = false;
                backward_dist(false);
            }
        }
        if (!fact_ok) {
            status = ST_FACT_FAILED;
            break;
        }
        if (BOUNDED) pg_prev = gmax;
        // barrier update for the next iteration (IPOPT monotone rule, lagged; oracle solve_one_ip)
        const double mub_next = (XB && fmax(fmax(0.5 * gmax, cmax), cmplmu) <= kIpKappaEps * mub)
                                    ? fmax(kIpTolCompl / 20.0, fmin(kIpKappaMu * mub, pow(mub, kIpThetaMu)))
                                    : mub;

        MMPC_PHASE(3);
        if constexpr (DIST) {
#include "sqp_group_step.inc"
        } else {   // the serial path (sqp_group_serial.inc): its QP passes
            if (gl == 0) {
                for (int pass = 0;; ++pass) {
                    if (pass > 0) backward(pass);
                    if (!fact_ok) break;
                    resolve = false;
                    step_sweep(pass);
                    if (!BOUNDED || !resolve || pass + 1 >= kBoundPasses) break;
                }
            }
            fact_ok = group_bcast_i(fact_ok, gbase);
            dJ = group_bcast(dJ, gbase);
        }
        if (!fact_ok) {
            status = ST_FACT_FAILED;
            break;
        }
        __builtin_amdgcn_wave_barrier();
        MMPC_PHASE(4);
#include "sqp_group_linesearch.inc"
    }
    __builtin_amdgcn_wave_barrier();
    MMPC_PHASE(6);
    // ---- write back V (reference layout), stage-parallel ----
    double* Vout = p.V + inst * (int64_t)NV;
    for (int k = gl; k <= N; k += G) {
#pragma unroll
        for (int r = 0; r < NX; ++r) Vout[k * NS + r] = sX[k * NX + r];
        if (k < N) {
#pragma unroll
            for (int c = 0; c < NU; ++c) Vout[k * NS + NX + c] = sU[k * NU + c];
        }
    }
    if (p.u0_out && gl < NU) p.u0_out[inst * NU + gl] = sU[gl];
    if (gl == 0) {
        if (p.status) p.status[inst] = status;
        if (p.iters) p.iters[inst] = it;
        if (p.kkt) p.kkt[inst] = kkt;
    }
    MMPC_PHASE(7);
    MMPC_PHASE_FLUSH
