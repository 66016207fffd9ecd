// sqp_group_phase_a.inc -- phase A of an iteration of the 16-lane kernel (kernel text, included once by
// sqp_group_body.inc at the top of its iteration loop): stage evaluation, the barrier terms, the group reductions.
// expects: the spine's setup (LDS and workspace views, Q, R, Rm, up, lin and the linear-mode block, with_lin, yl, yu, mub)
//          and the fused trial's hand-over fwd_ready, J0n, c1n, cmaxn, nfn.
// defines: J0, c1, cmax, nonfinite, evalA, lsum, cmpl0, cmplmu; clears fwd_ready.
        // ---- A. stage-parallel: F_k, A_k/B_k blocks, defects, merit value ----
        double J0 = J0n, c1 = c1n, cmax = cmaxn;
        int nonfinite = nfn;
        const bool evalA = !fwd_ready;
        if (evalA) {
            J0 = 0.0;
            c1 = 0.0;
            cmax = 0.0;
            nonfinite = 0;
            with_lin(std::integral_constant<int, WD>{}, [&](auto lm_c) {
                constexpr int LM = decltype(lm_c)::value;
                for (int k0 = gl; k0 < N; k0 += WD * G) {
                    int kk[WD];
                    double x[WD][NX], u[WD][NU], xd[WD][NX], Fq[WD][SQ], Fqd[WD][FD], Fu[WD][FU];
#pragma unroll
                    for (int e = 0; e < WD; ++e) {
                        kk[e] = (e == 0 || k0 + e * G < N) ? k0 + e * G : k0;
#pragma unroll
                        for (int r = 0; r < NX; ++r) x[e][r] = sX[kk[e] * NX + r];
#pragma unroll
                        for (int c = 0; c < NU; ++c) u[e][c] = sU[kk[e] * NU + c];
                    }
                    group_model_w<Model, WD, LM, true, SQ, FD, FU>(lin, lFq, lFqd, lFu, lxd, lxs, up, x, u, xd, Fq, Fqd, Fu);
                    double cd[WD][NX], er[WD][NX];
#pragma unroll
                    for (int e = 0; e < WD; ++e) {
                        const int k = kk[e];
#pragma unroll
                        for (int i = 0; i < FQ; ++i) sFq[k * FQ + i] = h * Fq[e][i];
#pragma unroll
                        for (int i = 0; i < FD; ++i) sFqd[k * FD + i] = h * Fqd[e][i];
#pragma unroll
                        for (int i = 0; i < FU; ++i) sFu[k * FU + i] = h * Fu[e][i];
#pragma unroll
                        for (int r = 0; r < NX; ++r) {
                            const double F = fma(h, xd[e][r], x[e][r]);
                            sF[k * NX + r] = F;
                            cd[e][r] = F - sX[(k + 1) * NX + r];
                            sC[k * NX + r] = cd[e][r];
                            er[e][r] = F - tr[k * NX + r];
                        }
                    }
                    // the sums in stage order; a repeated stage leaves them as they were
#pragma unroll
                    for (int e = 0; e < WD; ++e) {
                        const int k = kk[e];
                        double Js = J0, cs = c1;
#pragma unroll
                        for (int r = 0; r < NX; ++r) {
                            const double c = cd[e][r];
                            cmax = fmax(cmax, fabs(c));
                            cs += fabs(c);
                            nonfinite |= !isfinite(c);
                            Js = fma(er[e][r] * Q[r], er[e][r], Js);
                        }
#pragma unroll
                        for (int c = 0; c < NU; ++c) {
                            const double um = (k == 0) ? up[c] : sU[(k - 1) * NU + c];
                            const double dif = u[e][c] - um;
                            Js = fma(dif * R[c], dif, fma(u[e][c] * Rm[c], u[e][c], Js));
                        }
                        const bool on = e == 0 || k0 + e * G < N;
                        J0 = on ? Js : J0;
                        c1 = on ? cs : c1;
                    }
                }
            });
        }
        double lsum = 0.0, cmpl0 = 0.0, cmplmu = 0.0;  // interior point: sum log s, max |s z|, max |s z - mu|
        if constexpr (XB) {
            for (int k = gl; k < N; k += G) {
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    const double y = j < NX ? sX[(k + 1) * NX + j] : sU[k * NU + j - NX];
                    double sg, bb, zg;
                    ip_terms(y, yl[j], yu[j], sZl[k * NS + j], sZu[k * NS + j], mub, sg, bb, zg, cmpl0, cmplmu, lsum);
                    sSg[k * NS + j] = sg;
                    if constexpr (MEHR) sBb[k * NS + j] = 0.0;   // the affine predictor's barrier gradient
                    else sBb[k * NS + j] = bb;
                    sZg[k * NS + j] = zg;
                }
            }
            lsum = group_sum(lsum);
            cmpl0 = group_max(cmpl0);
            cmplmu = group_max(cmplmu);
            nonfinite |= !isfinite(lsum);
            // Sigma, b, z_u - z_l of every stage (HBM workspace) visible to the other lanes' serial sweeps
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        if (evalA) {
            J0 = group_sum(J0);
            c1 = group_sum(c1);
            cmax = group_max(cmax);
        }
        fwd_ready = false;
        __builtin_amdgcn_wave_barrier();
