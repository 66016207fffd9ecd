// sqp_group_wpass.inc -- the exact-Hessian W pass of the 16-lane kernel (kernel text, included once by
// sqp_group_body.inc behind the stop test): W_k of every stage, to the workspace or (WLDS) to the packed LDS record.
// expects: the spine's setup (wH, sW, PK, HW, WLDS, CAFF, w_zeros_stored) and lam in sD (adjoint_dist).
// defines: nothing that outlives it (w_stages, w_pair are local to its block); sets w_zeros_stored.
        if constexpr (EXACT) {
            // stage-parallel: W_k = h sum_s lam_{k+1,NQ+s} d^2 acc_s/d(x_k,u_k)^2 (lam from the adjoint, in sD)
            __builtin_amdgcn_wave_barrier();
            // W_k of stage k on lane k mod 16.  WLDS: the packed record goes to sW[k], over sD[1..] | sDX | sDU.  Record k
            // starts at double NX + PK k of sD and lam_{k'+1} ends at NX (k' + 2), so with PK >= NX writing record k can
            // only overwrite the lam operands of stages k' >= k.  The stages are therefore taken in rounds of 16 from the
            // last round down, for every N: the stages above a round are done, and within a round every lane's lam loads
            // precede every lane's stores in program order (one wave; LDS serves its accesses in order).
            // PAIR: a lane takes the stages k0 + gl and k0 + G + gl of two rounds together (kk[0], kk[1]; the first again when
            // the second is past the horizon), from the last pair of rounds down.  The argument holds for the pair as for
            // the round: the pairs of rounds above are done; inside the pair every lane's lam loads of BOTH stages precede
            // every lane's stores in program order, and the stores reach only lam operands of stages >= the pair's lowest,
            // all of them loaded or done.  A repeated stage stores its record twice, with the same values.
            auto w_stages = [&](const int (&kk)[WD]) {
                double x[WD][NX], u[WD][NU], la[WD][NA], W[WD][NS * NS];
#pragma unroll
                for (int e = 0; e < WD; ++e) {
                    const int k = kk[e];
#pragma unroll
                    for (int r2 = 0; r2 < NX; ++r2) x[e][r2] = sX[k * NX + r2];
#pragma unroll
                    for (int c = 0; c < NU; ++c) u[e][c] = sU[k * NU + c];
#pragma unroll
                    for (int s2 = 0; s2 < NA; ++s2) la[e][s2] = h * sD[(k + 1) * NX + NQ + s2];
                }
                if constexpr (WLDS) __builtin_amdgcn_wave_barrier();   // (compiler: no store of this round above a load)
                if constexpr (WD == 1) {
                    Model::eval_hess(x[0], u[0], la[0], W[0]);
                } else {   // the WD evaluations with their chains in turn (two_link_fast.h)
                    using T = dpack<WD>;
                    T xw[NX], uw[NU], lw[NA], Ww[NS * NS];
#pragma unroll
                    for (int e = 0; e < WD; ++e) {
#pragma unroll
                        for (int i = 0; i < NX; ++i) xw[i].v[e] = x[e][i];
#pragma unroll
                        for (int i = 0; i < NU; ++i) uw[i].v[e] = u[e][i];
#pragma unroll
                        for (int i = 0; i < NA; ++i) lw[i].v[e] = la[e][i];
                    }
                    Model::eval_hess(xw, uw, lw, Ww);
#pragma unroll
                    for (int e = 0; e < WD; ++e)
#pragma unroll
                        for (int i = 0; i < NS * NS; ++i) W[e][i] = Ww[i].v[e];
                }
#pragma unroll
                for (int e = 0; e < WD; ++e) {
                    const int k = kk[e];
                    if constexpr (WLDS) {
                        static_assert(!WLDS || PK >= NX, "write order of the W pass");
#pragma unroll
                        for (int r2 = 0; r2 < NX; ++r2)
#pragma unroll
                            for (int j = r2; j < NS; ++j)
                                if (WPack<Model>::idx(r2, j) >= 0) sW[k * PK + WPack<Model>::idx(r2, j)] = W[e][r2 * NS + j];
                    } else {
                        double* const dst = wH + k * HW;
#pragma unroll
                        for (int r2 = 0; r2 < NX; ++r2)
#pragma unroll
                            for (int j = 0; j < NS; ++j)
                                if (!w_struct_zero<Model>(r2, j) || !w_zeros_stored) dst[r2 * NS + j] = W[e][r2 * NS + j];
                        if constexpr (!CAFF) {
#pragma unroll
                            for (int a = 0; a < NU; ++a)
#pragma unroll
                                for (int b = 0; b < NU; ++b) dst[NX * NS + a * NU + b] = W[e][(NX + a) * NS + NX + b];
                        }
                    }
                }
            };
            auto w_pair = [&](int k0) {   // the lane's stages of the WD rounds from k0 (= its stage of the first)
                int kk[WD];
#pragma unroll
                for (int e = 0; e < WD; ++e) kk[e] = (e == 0 || k0 + e * G < N) ? k0 + e * G : k0;
                w_stages(kk);
            };
            if constexpr (WLDS) {
                for (int k0 = ((N - 1) / (WD * G)) * (WD * G); k0 >= 0; k0 -= WD * G)
                    if (k0 + gl < N) w_pair(k0 + gl);
                MMPC_PHASE(9);   // (timing build: "check" = the stop test and this W pass)
                // the records of the other lanes of this wave are in LDS before the sweep's loads: program order
                __builtin_amdgcn_wave_barrier();
            } else {
                for (int k = gl; k < N; k += WD * G) w_pair(k);
                w_zeros_stored = true;
                MMPC_PHASE(9);   // (timing build: "check" = the stop test and this W pass up to its fence)
                // the stores of the other lanes of this wave must be visible to the sweep's loads
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            }
        }
