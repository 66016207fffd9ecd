// sqp_group_dist_riccati.inc -- the lane-distributed Riccati sweeps (kernel text, included once by sqp_group_body.inc
// behind sqp_group_dist_grad.inc): lane r owns row r of P~ and p~.
// expects: the spine's setup, colA and load_acol (sqp_group_dist_grad.inc), fact_ok.
// defines: backward_dist(useW), the sweep of one QP solve; backward_vec(), its vector part alone for Mehrotra's corrector.
        auto backward_dist = [&](bool useW) {
            if constexpr (BOUNDED) {   // the hold targets (sHold) the gradient pass stored on every lane of this wave
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            }
            double Prow[NS], pvr;
            [[maybe_unused]] LdsB jcol = iAcN;   // load_acol's running address
            const double lxm = lx ? 1.0 : 0.0;
            // W_k row rx and uu block, loaded one stage ahead into one buffer: from the workspace, or (WLDS) row rx of
            // the packed record in LDS at this lane's row offset wrow + col(j), a structural zero under wm = 0;
            // the records were written by the other lanes of this wave, and LDS serves a wave's accesses in order.
            // (Round 2 used two
            // buffers two stages ahead; once the control-affine sweep dropped the uu block, the second buffer's
            // registers cost more than the load latency it hid: 0.1875 -> 0.1808 ms with one buffer, DESIGN.md 4c.)
            struct Wb {
                double r[NS], u[NU * NU];
            };
            Wb w0;
            auto load_w = [&](int k, Wb& b) {
#pragma unroll
                for (int j = 0; j < NS; ++j)   // row rx; masked at its uses
                    b.r[j] = WLDS ? sW[k * PK + wrow + WPack<Model>::col(j)] : wH[k * HW + rx * NS + j];
                if constexpr (!CAFF) {
#pragma unroll
                    for (int j = 0; j < NU * NU; ++j) b.u[j] = wH[k * HW + NX * NS + j];
                }
            };
            if (EXACT && useW) {
                load_w(N - 1, w0);
            }
#pragma unroll
            for (int j = 0; j < NS; ++j) Prow[j] = j < NX ? qoh[j] : 0.0;   // P~_N = blkdiag(Q, 0)
            pvr = Qr * (lx ? sX[N * NX + rx] - tr[(N - 1) * NX + rx] : 0.0);   // Q (x_N - r_{N-1})
            if constexpr (XB) {   // barrier at x_N: Sigma on the diagonal, b in p~
                const double sgN = sSg[(N - 1) * NS + rx], bbN = sBb[(N - 1) * NS + rx];
#pragma unroll
                for (int j = 0; j < NX; ++j) Prow[j] = fma(dgx[j], sgN, Prow[j]);
                pvr = fma(lxm, bbN, pvr);
            }
            // The stage's first FMAs (T, mv) need P~'s row, which is in registers, and h da/du and c of the stage: LDS
            // returns a wave's reads in order and the wave has nothing else to issue at the stage's top, so whatever
            // is queued in front of those two is waited for in full.  LOPS: the two are handed over from the stage
            // before (Hb, loaded in the middle of that stage's P~ update, as the W row one stage ahead), and the stage's
            // other operands are read in place in the order of first use, those of colA / at_mul last.  (A buffer for
            // all of a stage's operands spills to AGPRs; the sweep is otherwise bound by issue slots.)
            struct Hb {
                double fu[FU], c[NX];
            };
            Hb h0;
            auto load_head = [&](int k, Hb& b) {
#pragma unroll
                for (int i = 0; i < FU; ++i) b.fu[i] = sFu[k * FU + i];
#pragma unroll
                for (int q = 0; q < NX; ++q) b.c[q] = sC[k * NX + q];
            };
            if constexpr (LOPS) load_head(N - 1, h0);
            // stage k; LAST = (k == 0), peeled so that the stages k >= 1 carry no k == 0 selects or branches
            // HEADK: a stage k <= 2 of a kernel with the head block, which takes its K | kff columns
            auto stage = [&](int k, auto last_c, auto head_c, Wb& wb, Hb& hb) {
                constexpr bool LAST = decltype(last_c)::value, HEADK = decltype(head_c)::value;
#if defined(MMPC_PHASE_TIMING) && defined(MMPC_PHASE_STAGES)
                const unsigned long long st_top = __builtin_amdgcn_s_memtime();
                __builtin_amdgcn_sched_barrier(0);
#endif
                double hFq[SQ], hFqd[FD], hFu[FU], cc[NX], u[NU], um[NU], acol[NA];
                if constexpr (!LOPS) {
#pragma unroll
                    for (int i = 0; i < FQ; ++i) hFq[i] = sFq[k * FQ + i];
#pragma unroll
                    for (int i = 0; i < FD; ++i) hFqd[i] = sFqd[k * FD + i];
                    load_head(k, hb);
                }
#pragma unroll
                for (int i = 0; i < FU; ++i) hFu[i] = hb.fu[i];
#pragma unroll
                for (int q = 0; q < NX; ++q) cc[q] = hb.c[q];
#if defined(MMPC_PHASE_TIMING) && defined(MMPC_PHASE_STAGES)
                // the stamp behind the arrival of the operands of T and mv (s_memtime's own result needs lgkmcnt(0):
                // in the order of the other models it also waits for the reads queued behind them)
#pragma unroll
                for (int i = 0; i < FU; ++i) asm volatile("" ::"v"(hFu[i]));
#pragma unroll
                for (int q = 0; q < NX; ++q) asm volatile("" ::"v"(cc[q]));
                __builtin_amdgcn_sched_barrier(0);
                if (gl == 0 && blockIdx.x < kPhaseWavePhases && k < 32) {
                    g_mmpc_phase_cycles[kPhaseStageLog + 128 * blockIdx.x + 32 * gi + k] = st_top;
                    g_mmpc_phase_cycles[kPhaseWaitLog + 128 * blockIdx.x + 32 * gi + k] = __builtin_amdgcn_s_memtime();
                }
                __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    u[c] = sU[k * NU + c];
                    um[c] = LAST ? up[c] : sU[(k - 1) * NU + c];
                }
                load_acol(k, jcol, acol);
                if constexpr (LOPS) {
#pragma unroll
                    for (int i = 0; i < FQ; ++i) hFq[i] = sFq[k * FQ + i];
#pragma unroll
                    for (int i = 0; i < FD; ++i) hFqd[i] = sFqd[k * FD + i];
                }
                // XB: the barrier pieces of this stage (u_k) and of x_k (stage k-1), loaded with the stage operands:
                // read at their uses, deep in the stage, their HBM latency was exposed
                double xsgu[XB ? NU : 1], xbbu[XB ? NU : 1], xsgx = 0.0, xbbx = 0.0;
                if constexpr (XB) {
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        xsgu[a] = sSg[k * NS + NX + a];
                        xbbu[a] = sBb[k * NS + NX + a];
                    }
                    if constexpr (!LAST) {
                        xsgx = sSg[(k - 1) * NS + rx];
                        xbbx = sBb[(k - 1) * NS + rx];
                    }
                }
                double exr = 0.0, duu = 0.0;
                if constexpr (!LAST) {
                    const double xk = sX[k * NX + rx], trm = tr[(k - 1) * NX + rx];
                    exr = xk - trm;   // non-x lanes: finite leftovers of the clamped row, masked by lxm in pn
                    duu = sU[k * NU + ru] - sU[(k - 1) * NU + ru];
                }
                double wr[NS], wu[NU * NU];
                if constexpr (EXACT) {
#pragma unroll
                    for (int j = 0; j < NS; ++j) wr[j] = useW ? wb.r[j] : 0.0;
#pragma unroll
                    for (int j = 0; j < NU * NU; ++j) wu[j] = (useW && !CAFF) ? wb.u[j] : 0.0;
                    if (!LAST && useW) load_w(k - 1, wb);
                }
                // T = P~ [B; I] (row r), mv = P~_x. c + p~ (row r)
                double T[NU], mv = pvr;
#pragma unroll
                for (int b = 0; b < NU; ++b) {
                    double t = Prow[NX + b];
#pragma unroll
                    for (int s2 = 0; s2 < NA; ++s2) t = fma(Prow[NQ + s2], hFu[s2 * NU + b], t);
                    T[b] = t;
                }
#pragma unroll
                for (int q = 0; q < NX; ++q) mv = fma(Prow[q], cc[q], mv);
                double Tb[NS][NU], mvb[NS];
                sfor<0, NS>([&](auto I) {
#pragma unroll
                    for (int b = 0; b < NU; ++b) Tb[I][b] = row_bcast<I>(T[b]);
                    mvb[I] = row_bcast<I>(mv);
                });
                // H_ww = B^T P_xx B + B^T P_xu + P_ux B + P_uu + R + Rm, h_w (redundant)
                double Hww[NU][NU], hw[NU];
#pragma unroll
                for (int a = 0; a < NU; ++a) {
#pragma unroll
                    for (int b = a; b < NU; ++b) {
                        double t = Tb[NX + a][b];
#pragma unroll
                        for (int s2 = 0; s2 < NA; ++s2) t = fma(hFu[s2 * NU + a], Tb[NQ + s2][b], t);
                        if (a == b) t += R[a] + Rm[a];
                        if constexpr (EXACT && !CAFF) t += wu[a * NU + b];
                        if constexpr (XB) {
                            if (a == b) t += xsgu[a];   // barrier Sigma of u_k
                        }
                        Hww[a][b] = t;
                        Hww[b][a] = t;
                    }
                    double t = fma(R[a], u[a] - um[a], fma(Rm[a], u[a], mvb[NX + a]));
#pragma unroll
                    for (int s2 = 0; s2 < NA; ++s2) t = fma(hFu[s2 * NU + a], mvb[NQ + s2], t);
                    if constexpr (XB) t += xbbu[a];   // barrier gradient b of u_k
                    hw[a] = t;
                }
                // column r of Y = [H_wx | -R | .]: x-lanes (A^T T)[r], u-lanes -R e_{r-NX}
                double Ycol[NU];
#pragma unroll
                for (int a = 0; a < NU; ++a) {
                    double tb[NX];
#pragma unroll
                    for (int q = 0; q < NX; ++q) tb[q] = Tb[q][a];
                    Ycol[a] = colA(T[a], acol, tb) - rdg[a];
                    // H_wx[a][r] += W_ux[a][r] (x-lanes; WLDS: the x-lanes whose entry is not a structural zero)
                    if constexpr (EXACT) Ycol[a] = fma(WLDS ? wm[NX + a] : lxm, wr[NX + a], Ycol[a]);
                }
                // BOUNDED: the un-held stage rows [H_wx | -R | H_ww | h_w] (lane j < NS: column j; lanes NS.. the H_ww
                // columns and h_w, the idle lanes duplicating h_w) -- the step sweep forms the multiplier of a held
                // control from them (primal-dual active set: release a hold whose multiplier points into the box)
                if constexpr (BOUNDED) {
#pragma unroll
                    for (int c0 = 0; c0 < NR; c0 += G) {   // column c0 + r; lanes past the row rewrite its last entry
                        const int col = c0 + r < NR ? c0 + r : NR - 1;
#pragma unroll
                        for (int a = 0; a < NU; ++a) {
                            double v = hw[a];
#pragma unroll
                            for (int b = 0; b < NU; ++b)
                                if (col == NS + b) v = Hww[a][b];
                            wRel[(k * NU + a) * NR + col] = col < NS ? Ycol[a] : v;
                        }
                    }
                }
                // held controls (BOUNDED, sHold of this QP solve): du_a = target - u_a fixed in the stage QP, as the
                // one-lane sweep -- p~ gains [H_wx | -R]^T delta, h_w the coupling H_ww delta, the held rows and
                // columns of H_ww become the identity and the held rows of [H_wx | -R] zero, so that K_a = 0 and
                // kff_a = delta_a exactly; Rk: the -R columns of the u-lanes with the held rows removed
                double pexr = 0.0, Rk[NU];
#pragma unroll
                for (int c = 0; c < NU; ++c) Rk[c] = R[c];
                if constexpr (BOUNDED) {
                    bool hd[NU];
                    double dl[NU], hw2[NU];
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        const double tg = sHold[k * NU + a];
                        hd[a] = tg == tg;
                        dl[a] = hd[a] ? tg - u[a] : 0.0;
                        pexr = fma(Ycol[a], dl[a], pexr);
                    }
#pragma unroll
                    for (int b = 0; b < NU; ++b) {
                        double t = hw[b];
#pragma unroll
                        for (int a = 0; a < NU; ++a) t = fma(Hww[a][b], dl[a], t);
                        hw2[b] = hd[b] ? -dl[b] : t;
                    }
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        hw[a] = hw2[a];
#pragma unroll
                        for (int b = 0; b < NU; ++b)
                            if (hd[a] || hd[b]) Hww[a][b] = (a == b) ? 1.0 : 0.0;
                        if (hd[a]) {
                            Ycol[a] = 0.0;
                            Rk[a] = 0.0;
                        }
                    }
                }
                // Kcol = H_ww^-1 Ycol (this lane's column of K~), kff = H_ww^-1 h_w (redundant)
                double Kcol[NU], kff[NU], Ku[NU][NU];
                // XB: Cholesky H_ww = L L^T, Ytil = L^-1 Ycol (this lane's column of L^-1 [H_wx | -R]), htil = L^-1 h_w;
                // the update P~ -= Ytil^T Ytil stays positive semidefinite under the barrier's large Sigma
                double Ytil[NU], htil[NU];
                if constexpr (XB) {
                    double Ld[NU][NU], il[NU];
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        double sd = Hww[a][a];
#pragma unroll
                        for (int q = 0; q < a; ++q) sd = fma(-Ld[a][q], Ld[a][q], sd);
                        fact_ok &= (sd > 0.0) && isfinite(sd);
                        const double sp = fmax(sd, 1e-300);
                        double rr = __builtin_amdgcn_rsq(sp);
                        rr = rr * fma(-0.5 * sp * rr, rr, 1.5);
                        rr = rr * fma(-0.5 * sp * rr, rr, 1.5);
                        Ld[a][a] = sp * rr;
                        il[a] = rr;
#pragma unroll
                        for (int b = a + 1; b < NU; ++b) {
                            double t = Hww[a][b];
#pragma unroll
                            for (int q = 0; q < a; ++q) t = fma(-Ld[b][q], Ld[a][q], t);
                            Ld[b][a] = t * il[a];
                        }
                    }
#pragma unroll
                    for (int a = 0; a < NU; ++a) {   // forward substitutions
                        double t = Ycol[a], th = hw[a];
#pragma unroll
                        for (int q = 0; q < a; ++q) {
                            t = fma(-Ld[a][q], Ytil[q], t);
                            th = fma(-Ld[a][q], htil[q], th);
                        }
                        Ytil[a] = t * il[a];
                        htil[a] = th * il[a];
                    }
#pragma unroll
                    for (int a = NU - 1; a >= 0; --a) {   // back substitutions: K~ column, kff
                        double t = Ytil[a], th = htil[a];
#pragma unroll
                        for (int q = a + 1; q < NU; ++q) {
                            t = fma(-Ld[q][a], Kcol[q], t);
                            th = fma(-Ld[q][a], kff[q], th);
                        }
                        Kcol[a] = t * il[a];
                        kff[a] = th * il[a];
                    }
                    if constexpr (MEHR) {   // the record of this stage for backward_vec
                        double* const rec = sVr + k * VR;
                        double pc = 0.0;
#pragma unroll
                        for (int q = 0; q < NX; ++q) pc = fma(Prow[q], cc[q], pc);
                        rec[r] = pc;
                        rec[G + r] = fma(-Rr, duu, lxm * (Qr * exr));
#pragma unroll
                        for (int a = 0; a < NU; ++a) {
                            rec[(2 + a) * G + r] = Ytil[a];
#pragma unroll
                            for (int q = 0; q < a; ++q) rec[VL * G + a * (a + 1) / 2 + q] = Ld[a][q];
                            rec[VL * G + a * (a + 1) / 2 + a] = il[a];
                            rec[VL * G + VC + a] = fma(R[a], u[a] - um[a], Rm[a] * u[a]);
                        }
                    }
                } else if constexpr (NU == 2) {
                    const double det = fma(Hww[0][0], Hww[1][1], -Hww[0][1] * Hww[0][1]);
                    fact_ok &= (Hww[0][0] > 0.0) && (det > 0.0) && isfinite(det);
                    const double idet = rcp_nr(det);
                    const double i00 = Hww[1][1] * idet, i11 = Hww[0][0] * idet, i01 = -Hww[0][1] * idet;
                    Kcol[0] = fma(i00, Ycol[0], i01 * Ycol[1]);
                    Kcol[1] = fma(i01, Ycol[0], i11 * Ycol[1]);
                    kff[0] = fma(i00, hw[0], i01 * hw[1]);
                    kff[1] = fma(i01, hw[0], i11 * hw[1]);
                    Ku[0][0] = -i00 * Rk[0];
                    Ku[0][1] = -i01 * Rk[1];
                    Ku[1][0] = -i01 * Rk[0];
                    Ku[1][1] = -i11 * Rk[1];
                } else {   // Cholesky H_ww = L L^T (rsq + Newton), solves with L and L^T
                    double Ld[NU][NU], il[NU];
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        double sd = Hww[a][a];
#pragma unroll
                        for (int q = 0; q < a; ++q) sd = fma(-Ld[a][q], Ld[a][q], sd);
                        fact_ok &= (sd > 0.0) && isfinite(sd);
                        const double sp = fmax(sd, 1e-300);
                        double rr = __builtin_amdgcn_rsq(sp);
                        rr = rr * fma(-0.5 * sp * rr, rr, 1.5);
                        rr = rr * fma(-0.5 * sp * rr, rr, 1.5);
                        Ld[a][a] = sp * rr;
                        il[a] = rr;
#pragma unroll
                        for (int b = a + 1; b < NU; ++b) {
                            double t = Hww[a][b];
#pragma unroll
                            for (int q = 0; q < a; ++q) t = fma(-Ld[b][q], Ld[a][q], t);
                            Ld[b][a] = t * il[a];
                        }
                    }
                    auto chol_solve = [&](const double* rhs, double* out) {
                        double y[NU];
#pragma unroll
                        for (int a = 0; a < NU; ++a) {
                            double t = rhs[a];
#pragma unroll
                            for (int q = 0; q < a; ++q) t = fma(-Ld[a][q], y[q], t);
                            y[a] = t * il[a];
                        }
#pragma unroll
                        for (int a = NU - 1; a >= 0; --a) {
                            double t = y[a];
#pragma unroll
                            for (int q = a + 1; q < NU; ++q) t = fma(-Ld[q][a], out[q], t);
                            out[a] = t * il[a];
                        }
                    };
                    chol_solve(Ycol, Kcol);
                    chol_solve(hw, kff);
#pragma unroll
                    for (int c = 0; c < NU; ++c) {   // column NX + c of K~: H_ww^-1 (-R_c e_c)
                        double e[NU], o[NU];
#pragma unroll
                        for (int a = 0; a < NU; ++a) e[a] = (a == c) ? -Rk[c] : 0.0;
                        chol_solve(e, o);
#pragma unroll
                        for (int a = 0; a < NU; ++a) Ku[a][c] = o[a];
                    }
                }
                // [K_k | kff_k] = -[K~ | kff~] (lane j < NS stores column j, lanes >= NS the feed-forward column: kff
                // is computed redundantly, bit-identical on every lane of the group, so the duplicate stores of the
                // idle lanes write the same value -- no exec-mask branch in the sweep)
                {
                    const int col = r < NS ? r : NS;
#pragma unroll
                    for (int a = 0; a < NU; ++a)
                        (HEADK ? sKh : wK)[(k * NU + a) * (NS + 1) + col] = -(r < NS ? Kcol[a] : kff[a]);
                }
                if constexpr (LAST) return;
                // A^T P_xx A (row r) from the broadcast P_xx, p~_x = A^T mv + Q (x_k - r_{k-1})
                double Pb[NX][NX];
                sfor<0, NX>([&](auto I) {
#pragma unroll
                    for (int j = I; j < NX; ++j) {
                        Pb[I][j] = row_bcast<I>(Prow[j]);
                        Pb[j][I] = Pb[I][j];
                    }
                });
                double Ur[NX], Pn[NX];
#pragma unroll
                for (int j = 0; j < NX; ++j) {
                    double pc[NX];
#pragma unroll
                    for (int q = 0; q < NX; ++q) pc[q] = Pb[q][j];
                    Ur[j] = colA(Prow[j], acol, pc);
                }
                at_mul<NQ, NA, double>(h, hFq, hFqd, Ur, Pn);
                // the next stage's h da/du and c: T, mv, H_ww and h_w of this stage are formed, so the buffer is free, and
                // the rest of the P~ update (some 60 instructions) covers the reads.  Left alone, the scheduler sinks
                // them to their uses at the next stage's top; the barrier further up in the stage (in front of the
                // P~ update, or of Y) made the unbounded exact kernel spill.
                if constexpr (LOPS) {
                    load_head(k - 1, hb);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // x-lanes A^T mv + Q (x_k - r_{k-1}), u-lanes -R (u_k - u_{k-1}), idle lanes 0 -- blended with the
                // lane-role factor (Rr = 0 off the u-lanes) instead of a branch
                double pn = fma(-Rr, duu, lxm * fma(Qr, exr, colA(mv, acol, mvb)));
                double sgk = 0.0;   // XB: barrier Sigma and b of x_k (stage k-1's y)
                if constexpr (XB) {
                    sgk = xsgx;
                    pn = fma(lxm, xbbx, pn);
                }
                if constexpr (XB) {   // P~_k = blkdiag(A^T P_xx A + Q + Sigma, R) - Ytil^T Ytil, p~_k = pn - Ytil^T htil
                    double Yb[NU][NS];
                    sfor<0, NS>([&](auto I) {
#pragma unroll
                        for (int a = 0; a < NU; ++a) Yb[a][I] = row_bcast<I>(Ytil[a]);
                    });
#pragma unroll
                    for (int j = 0; j < NS; ++j) {
                        double v = j < NX ? fma(dgx[j], sgk, Pn[j] + qoh[j]) : rdg[j - NX];
                        if constexpr (EXACT) {
                            if (j < NX) v = fma(lxm, wr[j], v);   // + W_xx row r (round 6: the exact Hessian under bounds)
                        }
#pragma unroll
                        for (int a = 0; a < NU; ++a) v = fma(-Ytil[a], Yb[a][j], v);
                        Prow[j] = v;
                    }
                    double pv2 = pn;
#pragma unroll
                    for (int a = 0; a < NU; ++a) pv2 = fma(-Ytil[a], htil[a], pv2);
                    pvr = pv2;
                    return;
                }
                // K~ columns of the other lanes
                double Kb[NU][NX];
                sfor<0, NX>([&](auto I) {
#pragma unroll
                    for (int a = 0; a < NU; ++a) Kb[a][I] = row_bcast<I>(Kcol[a]);
                });
                // P~_k = blkdiag(A^T P_xx A + Q, R) - Y^T K~, p~_k = pn - Y^T kff (row r)
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    double v = j < NX ? Pn[j] + qoh[j] : rdg[j - NX];
                    if constexpr (EXACT) {
                        if (j < NX) v = fma(WLDS ? wm[j] : lxm, wr[j], v);   // W_xx row r (x-lanes; the mask folded into the add)
                    }
#pragma unroll
                    for (int a = 0; a < NU; ++a) v = fma(-Ycol[a], j < NX ? Kb[a][j] : Ku[a][j - NX], v);
                    Prow[j] = v;
                }
                double pv2 = pn;
#pragma unroll
                for (int a = 0; a < NU; ++a) pv2 = fma(-Ycol[a], kff[a], pv2);
                if constexpr (BOUNDED) pv2 += pexr;
                pvr = pv2;
            };
            // inner stages N-1 .. 1 by unconditional pairs (an odd count peels stage N-1 in front), as the step sweep;
            // the control-bounded sweep one stage per trip (its hold logic and relaxation rows fill the registers: two
            // stages in flight spilled to scratch inside the loop)
            using F_ = std::false_type;
            using T_ = std::true_type;
            if constexpr (BOUNDED || (XB && EXACT)) {
                for (int k = N - 1; k >= 1; --k) stage(k, F_{}, F_{}, w0, h0);
                stage(0, T_{}, F_{}, w0, h0);
            } else if constexpr (KH > 0) {
                // head block: the pair loop ends at stage 3 (an odd count of stages N - 1 .. 3 peels stage N - 1), and
                // the stages 2, 1 (one more pair body) and 0 that store there follow as straight-line code -- a store
                // address chosen per stage inside the loop would cost every stage what these three save.  (Stages
                // 2 and 1 each under a test of their own made the exact kernel spill four registers.)
                int k = N - 1;
                if (N >= 4 && ((N - 3) & 1)) stage(k--, F_{}, F_{}, w0, h0);
                for (; k >= 4; k -= 2) {
                    stage(k, F_{}, F_{}, w0, h0);
                    stage(k - 1, F_{}, F_{}, w0, h0);
                }
                if (N >= 3) {
                    stage(2, F_{}, T_{}, w0, h0);
                    stage(1, F_{}, T_{}, w0, h0);
                } else if (N == 2) {
                    stage(1, F_{}, T_{}, w0, h0);
                }
                stage(0, T_{}, T_{}, w0, h0);
            } else if ((N - 1) & 1) {
                stage(N - 1, F_{}, F_{}, w0, h0);
                for (int k = N - 2; k >= 2; k -= 2) {
                    stage(k, F_{}, F_{}, w0, h0);
                    stage(k - 1, F_{}, F_{}, w0, h0);
                }
                stage(0, T_{}, F_{}, w0, h0);
            } else {
                for (int k = N - 1; k >= 2; k -= 2) {
                    stage(k, F_{}, F_{}, w0, h0);
                    stage(k - 1, F_{}, F_{}, w0, h0);
                }
                stage(0, T_{}, F_{}, w0, h0);
            }
        };
        // MEHR corrector: the vector part (p~, kff) of the Riccati recursion for the barrier gradient now in sBb, on the
        // matrices of the sweep that just ran (its per-stage record sVr): mv = p~ + P~_x c, h_w, kff = H_ww^-1 h_w through
        // the stored factor, p~_k = pn - Ytil^T L^-1 h_w.  Only the kff column of the gains is rewritten.
        [[maybe_unused]] auto backward_vec = [&]() {
            if constexpr (MEHR) {
                const double lxm = lx ? 1.0 : 0.0;
                [[maybe_unused]] LdsB jcol = iAcN;   // load_acol's running address
                double pvr = Qr * (lx ? sX[N * NX + rx] - tr[(N - 1) * NX + rx] : 0.0);   // Q (x_N - r_{N-1})
                pvr = fma(lxm, sBb[(N - 1) * NS + rx], pvr);
                struct Rec {
                    double pc, pn0, yt[NU], sh[VS], bbu[NU], bbx;
                };
                auto fetch = [&](int k, Rec& o) {
                    const double* const rec = sVr + k * VR;
                    o.pc = rec[r];
                    o.pn0 = rec[G + r];
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        o.yt[a] = rec[(2 + a) * G + r];
                        o.bbu[a] = sBb[k * NS + NX + a];
                    }
#pragma unroll
                    for (int i = 0; i < VS; ++i) o.sh[i] = rec[VL * G + i];
                    o.bbx = sBb[(k > 0 ? k - 1 : 0) * NS + rx];   // b of x_k (stage k - 1's y); unused at k = 0
                };
                auto stage = [&](int k, const Rec& o) {
                    double hFu[FU], acol[NA];
#pragma unroll
                    for (int i = 0; i < FU; ++i) hFu[i] = sFu[k * FU + i];
                    load_acol(k, jcol, acol);
                    const double mv = pvr + o.pc;
                    double mvb[NS];
                    sfor<0, NS>([&](auto I) { mvb[I] = row_bcast<I>(mv); });
                    double htil[NU], kff[NU];
#pragma unroll
                    for (int a = 0; a < NU; ++a) {   // h_w, then L^-1 h_w
                        double t = o.sh[VC + a] + mvb[NX + a];
#pragma unroll
                        for (int s2 = 0; s2 < NA; ++s2) t = fma(hFu[s2 * NU + a], mvb[NQ + s2], t);
                        t += o.bbu[a];
#pragma unroll
                        for (int q = 0; q < a; ++q) t = fma(-o.sh[a * (a + 1) / 2 + q], htil[q], t);
                        htil[a] = t * o.sh[a * (a + 1) / 2 + a];
                    }
#pragma unroll
                    for (int a = NU - 1; a >= 0; --a) {
                        double t = htil[a];
#pragma unroll
                        for (int q = a + 1; q < NU; ++q) t = fma(-o.sh[q * (q + 1) / 2 + a], kff[q], t);
                        kff[a] = t * o.sh[a * (a + 1) / 2 + a];
                    }
                    // bit-identical on every lane: duplicate stores, no exec-mask branch (as backward_dist)
#pragma unroll
                    for (int a = 0; a < NU; ++a) wK[(k * NU + a) * (NS + 1) + NS] = -kff[a];
                    if (k == 0) return;
                    double pv2 = fma(lxm, colA(mv, acol, mvb) + o.bbx, o.pn0);
#pragma unroll
                    for (int a = 0; a < NU; ++a) pv2 = fma(-o.yt[a], htil[a], pv2);
                    pvr = pv2;
                };
                // two buffers, each refilled one stage ahead of its use
                Rec o0, o1;
                fetch(N - 1, o0);
                int k = N - 1;
                for (; k >= 1; k -= 2) {
                    fetch(k - 1, o1);
                    stage(k, o0);
                    fetch(k >= 2 ? k - 2 : 0, o0);
                    stage(k - 1, o1);
                }
                if (k == 0) stage(0, o0);
            }
        };
