// sqp_group_serial.inc -- the one-lane serial sweeps of the 16-lane kernel (kernel text, included once by
// sqp_group_body.inc): the sweeps that only the models with nx + nu >= 16 run (!DIST), on the first lane of the group.
// No lane-distributed code is in here.  Their callers stay in the spine, in its two `!DIST` branches (the d recursion
// with backward(0), and the QP-pass loop): as lambdas in this file they changed those kernels' code (DESIGN.md 4c).
// expects: the spine's setup and, of this iteration, nonfinite (phase A), gmax, lmax, fact_ok, beps.
// defines: backward(pass), step_sweep(pass), and between them (their place in the order of definitions) dJ and resolve,
//          which the lane-distributed step writes too.
        // backward sweep of QP solve `pass` (gradient and stop-test quantities are the same in every pass)
        auto backward = [&](int pass) {
            // P~ (symmetric, upper triangle used) and p~ on s = [dx_k; du_{k-1}]; P~_N = blkdiag(Q, 0)
            double P[NS][NS], pv[NS], lam[NX], unext[NU];
#define Ps(i, j) ((i) <= (j) ? P[(i)][(j)] : P[(j)][(i)])
#pragma unroll
            for (int a = 0; a < NS; ++a) {
                pv[a] = 0.0;
#pragma unroll
                for (int b = a; b < NS; ++b) P[a][b] = (a == b && a < NX) ? Q[a] : 0.0;
            }
#pragma unroll
            for (int r = 0; r < NX; ++r) {
                const double eb = sX[N * NX + r] - tr[(N - 1) * NX + r];  // x_N - r_{N-1}
                pv[r] = Q[r] * eb;
                lam[r] = Q[r] * (sD[N * NX + r] + eb);  // lam_N = Q e_{N-1}
                if constexpr (XB) {  // barrier at x_N: Sigma, b in the value function, z_u - z_l in the adjoint
                    P[r][r] += sSg[(N - 1) * NS + r];
                    pv[r] += sBb[(N - 1) * NS + r];
                    lam[r] += sZg[(N - 1) * NS + r];
                }
                lmax = fmax(lmax, fabs(lam[r]));
            }
#pragma unroll
            for (int c = 0; c < NU; ++c) unext[c] = 0.0;
            for (int k = N - 1; k >= 0; --k) {
                const double* hFq = sFq + k * FQ;
                const double* hFqd = sFqd + k * FD;
                double hFu[FU], x[NX], u[NU], um[NU], cc[NX], tg[NU];
#pragma unroll
                for (int i = 0; i < FU; ++i) hFu[i] = sFu[k * FU + i];
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    x[r] = sX[k * NX + r];
                    cc[r] = sC[k * NX + r];
                }
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    u[c] = sU[k * NU + c];
                    um[c] = (k == 0) ? up[c] : sU[(k - 1) * NU + c];
                }
                // reduced gradient g_k = B_k^T lam_{k+1} + R/Rm terms
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    double g = 0.0;
#pragma unroll
                    for (int s = 0; s < NA; ++s) g = fma(hFu[s * NU + c], lam[NQ + s], g);
                    g = fma(R[c], u[c] - um[c], fma(Rm[c], u[c], g));
                    if (k + 1 < N) g -= R[c] * (unext[c] - u[c]);
                    if (XB) g += sZg[k * NS + NX + c];  // reduced Lagrangian gradient
                    if (!BOUNDED) {
                        gmax = fmax(gmax, fabs(2.0 * g));
                    } else {  // projected gradient; hold rule (pass 0) or the holds of the previous solve
                        gmax = fmax(gmax, fabs(u[c] - proj(u[c] - 2.0 * g, lbv[c], ubv[c])));
                        if (pass == 0) {
                            tg[c] = (u[c] <= lbv[c] + beps && g > 0.0)   ? lbv[c]
                                    : (u[c] >= ubv[c] - beps && g < 0.0) ? ubv[c]
                                                                          : NAN;
                            sHold[k * NU + c] = tg[c];
                        } else {
                            tg[c] = sHold[k * NU + c];
                        }
                    }
                    nonfinite |= !isfinite(g);
                    unext[c] = u[c];
                }
                // adjoint lam_k = Q e_{k-1} + A_k^T lam_{k+1},  e_{k-1} = d_k + x_k - r_{k-1}
                if (k >= 1) {
                    double ln[NX];
                    at_mul<NQ, NA, double>(h, hFq, hFqd, lam, ln);
#pragma unroll
                    for (int r = 0; r < NX; ++r) {
                        lam[r] = fma(Q[r], sD[k * NX + r] + x[r] - tr[(k - 1) * NX + r], ln[r]);
                        if (XB) lam[r] += sZg[(k - 1) * NS + r];
                        lmax = fmax(lmax, fabs(lam[r]));
                    }
                }
                // Riccati step (sqp_lane.h): G = P_xx B + P_xu, H_ww, h_w, Y = L^-1 [H_wx | -R | h_w]
                double Gm[NX][NU];
#pragma unroll
                for (int r = 0; r < NX; ++r)
#pragma unroll
                    for (int c = 0; c < NU; ++c) {
                        double t = Ps(r, NX + c);
#pragma unroll
                        for (int s = 0; s < NA; ++s) t = fma(Ps(r, NQ + s), hFu[s * NU + c], t);
                        Gm[r][c] = t;
                    }
                double mv[NX];
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    double t = pv[r];
#pragma unroll
                    for (int q = 0; q < NX; ++q) t = fma(Ps(r, q), cc[q], t);
                    mv[r] = t;
                }
                double Hww[NU][NU], Y[NU][NS + 1];
#pragma unroll
                for (int a = 0; a < NU; ++a) {
#pragma unroll
                    for (int b = a; b < NU; ++b) {
                        double t = Ps(NX + a, NX + b);
#pragma unroll
                        for (int s = 0; s < NA; ++s)
                            t = fma(hFu[s * NU + a], Gm[NQ + s][b], fma(Ps(NQ + s, NX + a), hFu[s * NU + b], t));
                        if (a == b) t += R[a] + Rm[a];
                        if (XB && a == b) t += sSg[k * NS + NX + a];
                        Hww[a][b] = t;
                    }
                    double t = fma(R[a], u[a] - um[a], fma(Rm[a], u[a], pv[NX + a]));
                    if (XB) t += sBb[k * NS + NX + a];
#pragma unroll
                    for (int s = 0; s < NA; ++s) t = fma(hFu[s * NU + a], mv[NQ + s], t);
#pragma unroll
                    for (int r = 0; r < NX; ++r) t = fma(Ps(r, NX + a), cc[r], t);
                    Y[a][NS] = t;
                    double ga[NX];
#pragma unroll
                    for (int r = 0; r < NX; ++r) ga[r] = Gm[r][a];
                    at_mul<NQ, NA, double>(h, hFq, hFqd, ga, &Y[a][0]);
#pragma unroll
                    for (int c = 0; c < NU; ++c) Y[a][NX + c] = (a == c) ? -R[a] : 0.0;
                }
                // held controls (bounded): w_A = target - u fixed in the stage QP, as sqp_lane.h
                double pex[NS];
                if (BOUNDED) {
                    bool hd[NU], any = false;
                    double dl[NU];
#pragma unroll
                    for (int j = 0; j < NS; ++j) pex[j] = 0.0;
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        hd[a] = tg[a] == tg[a];
                        dl[a] = hd[a] ? tg[a] - u[a] : 0.0;
                        any |= hd[a];
                    }
                    if (any) {
#pragma unroll
                        for (int a = 0; a < NU; ++a)
#pragma unroll
                            for (int j = 0; j < NS; ++j) pex[j] = fma(Y[a][j], dl[a], pex[j]);
#pragma unroll
                        for (int b = 0; b < NU; ++b) {
                            double t = Y[b][NS];
#pragma unroll
                            for (int a = 0; a < NU; ++a) t = fma(Hww[a < b ? a : b][a < b ? b : a], dl[a], t);
                            Y[b][NS] = hd[b] ? -dl[b] : t;
                        }
#pragma unroll
                        for (int a = 0; a < NU; ++a) {
#pragma unroll
                            for (int b = a; b < NU; ++b)
                                if (hd[a] || hd[b]) Hww[a][b] = (a == b) ? 1.0 : 0.0;
                            if (hd[a])
#pragma unroll
                                for (int j = 0; j < NS; ++j) Y[a][j] = 0.0;
                        }
                    }
                }
                // P~_k x block A^T P_xx A + Q and p~_k x part A^T mv + Q (x_k - r_{k-1}), before P is overwritten
                double Pn[NX][NX], pn[NS];
                if (k >= 1) {
#pragma unroll
                    for (int b = 0; b < NX; ++b) {
                        double row[NX], tcol[NX];
#pragma unroll
                        for (int r = 0; r < NX; ++r) {
                            double t;
                            if (b < NQ) {
                                t = Ps(r, b);
#pragma unroll
                                for (int s = 0; s < NA; ++s) t = fma(hFq[s * NQ + b], Ps(r, NQ + s), t);
                            } else {
                                t = (b - NQ < NQ) ? fma(h, Ps(r, b - NQ), Ps(r, b)) : Ps(r, b);
#pragma unroll
                                for (int s = 0; s < NA; ++s) t = fma(hFqd[s * NA + b - NQ], Ps(r, NQ + s), t);
                            }
                            tcol[r] = t;
                        }
                        at_mul<NQ, NA, double>(h, hFq, hFqd, tcol, row);
#pragma unroll
                        for (int a = 0; a <= b; ++a)
                            Pn[a][b] = row[a] + ((a == b) ? Q[a] + (XB ? sSg[(k - 1) * NS + a] : 0.0) : 0.0);
                    }
                    double t[NX];
                    at_mul<NQ, NA, double>(h, hFq, hFqd, mv, t);
#pragma unroll
                    for (int q = 0; q < NX; ++q) {
                        pn[q] = fma(Q[q], x[q] - tr[(k - 1) * NX + q], t[q]);
                        if (XB) pn[q] += sBb[(k - 1) * NS + q];
                    }
#pragma unroll
                    for (int c = 0; c < NU; ++c) pn[NX + c] = -R[c] * (u[c] - um[c]);
                }
                // [K_k | kff_k] = -H_ww^-1 [H_wx | -R | h_w] (into wK) and Y with Y^T Y = Z^T H_ww^-1 Z for the
                // update of P~ and p~.  nu = 2: explicit inverse (one reciprocal; no square roots -- the serial
                // sweep is latency-bound, DESIGN.md 4c); otherwise Cholesky, Y = L^-1 Z.
                double Kt[NU][NS + 1];
                if constexpr (NU == 2 && !XB) {  // XB: Cholesky (Y^T Y stays PSD with the large barrier Sigma)
                    const double det = fma(Hww[0][0], Hww[1][1], -Hww[0][1] * Hww[0][1]);
                    fact_ok &= (Hww[0][0] > 0.0) && (det > 0.0) && isfinite(det);
                    const double idet = rcp_nr(det);  // two Newton steps: ~1 ulp, off the division's long chain
                    const double i00 = Hww[1][1] * idet, i11 = Hww[0][0] * idet, i01 = -Hww[0][1] * idet;
#pragma unroll
                    for (int j = 0; j <= NS; ++j) {
                        Kt[0][j] = fma(i00, Y[0][j], i01 * Y[1][j]);
                        Kt[1][j] = fma(i01, Y[0][j], i11 * Y[1][j]);
                    }
                } else {
                    double Ld[NU][NU], il[NU];
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        double sd = Hww[a][a];
#pragma unroll
                        for (int q = 0; q < a; ++q) sd = fma(-Ld[a][q], Ld[a][q], sd);
                        fact_ok &= (sd > 0.0) && isfinite(sd);
                        // 1/sqrt by v_rsq + two Newton steps (no square root and division on the serial chain)
                        const double sp = fmax(sd, 1e-300);
                        double r = __builtin_amdgcn_rsq(sp);
                        r = r * fma(-0.5 * sp * r, r, 1.5);
                        r = r * fma(-0.5 * sp * r, r, 1.5);
                        Ld[a][a] = sp * r;
                        il[a] = r;
#pragma unroll
                        for (int b = a + 1; b < NU; ++b) {
                            double t = Hww[a][b];
#pragma unroll
                            for (int q = 0; q < a; ++q) t = fma(-Ld[b][q], Ld[a][q], t);
                            Ld[b][a] = t * il[a];
                        }
                    }
#pragma unroll
                    for (int a = 0; a < NU; ++a)
#pragma unroll
                        for (int j = 0; j <= NS; ++j) {
                            double t = Y[a][j];
#pragma unroll
                            for (int q = 0; q < a; ++q) t = fma(-Ld[a][q], Y[q][j], t);
                            Y[a][j] = t * il[a];
                        }
#pragma unroll
                    for (int a = NU - 1; a >= 0; --a)
#pragma unroll
                        for (int j = 0; j <= NS; ++j) {
                            double t = Y[a][j];
#pragma unroll
                            for (int q = a + 1; q < NU; ++q) t = fma(-Ld[q][a], Kt[q][j], t);
                            Kt[a][j] = t * il[a];
                        }
                }
#pragma unroll
                for (int a = 0; a < NU; ++a)
#pragma unroll
                    for (int j = 0; j <= NS; ++j) wK[(k * NU + a) * (NS + 1) + j] = -Kt[a][j];
                if (k == 0) break;
                // P~_k = blkdiag(A^T P_xx A + Q, R) - Z^T H_ww^-1 Z, p~_k = pn - Z^T H_ww^-1 h_w:
                // nu = 2 as Y^T Kt (Y = Z, Kt = H_ww^-1 Z), Cholesky as Y^T Y (Y = L^-1 Z)
                const double(&YB)[NU][NS + 1] = (NU == 2 && !XB) ? Kt : Y;
#pragma unroll
                for (int a = 0; a < NS; ++a) {
                    double t = pn[a];
#pragma unroll
                    for (int q = 0; q < NU; ++q) t = fma(-Y[q][a], YB[q][NS], t);
                    if (BOUNDED) t += pex[a];
                    pv[a] = t;
#pragma unroll
                    for (int b = a; b < NS; ++b) {
                        double v = (b < NX) ? Pn[a][b] : ((a == b) ? R[a - NX] : 0.0);
#pragma unroll
                        for (int q = 0; q < NU; ++q) v = fma(-Y[q][a], YB[q][b], v);
                        P[a][b] = v;
                    }
                }
            }
#undef Ps
        };
        // ---- C. one lane: step sweep du = K s + kff, dx, directional derivative ----
        double dJ = 0.0;
        bool resolve = false;
        auto step_sweep = [&](int pass) {
            dJ = 0.0;
            double dx[NX], dup[NU], um[NU];
#pragma unroll
            for (int r = 0; r < NX; ++r) {
                dx[r] = 0.0;
                sDX[r] = 0.0;
            }
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                dup[c] = 0.0;
                um[c] = up[c];
            }
            // software pipeline: K_{k+1} (HBM) and the LDS operands of step k+1 are loaded during step k
            constexpr int NK = NU * (NS + 1);
            double nK[NK], nFq[SQ], nFqd[FD], nFu[FU], nF[NX], nc[NX], nr[NX], nu_[NU];
#define GROUP_LOAD_STEP(k_)                                                                        \
        do {                                                                                           \
            const int kk_ = (k_);                                                                      \
            _Pragma("unroll") for (int i_ = 0; i_ < NK; ++i_) nK[i_] = wK[kk_ * NK + i_];              \
            _Pragma("unroll") for (int i_ = 0; i_ < FQ; ++i_) nFq[i_] = sFq[kk_ * FQ + i_];             \
            _Pragma("unroll") for (int i_ = 0; i_ < FD; ++i_) nFqd[i_] = sFqd[kk_ * FD + i_];           \
            _Pragma("unroll") for (int i_ = 0; i_ < FU; ++i_) nFu[i_] = sFu[kk_ * FU + i_];             \
            _Pragma("unroll") for (int r_ = 0; r_ < NX; ++r_) {                                        \
            nF[r_] = sF[kk_ * NX + r_];                                                            \
            nc[r_] = sC[kk_ * NX + r_];                                                            \
            nr[r_] = sR[kk_ * NX + r_];                                                            \
            }                                                                                          \
            _Pragma("unroll") for (int c_ = 0; c_ < NU; ++c_) nu_[c_] = sU[kk_ * NU + c_];             \
        } while (0)
            GROUP_LOAD_STEP(0);
            // unrolled by two so that the prefetch buffers are renamed instead of copied (2-link only: the exo
            // step spills when unrolled)
            constexpr int kStepUnroll = NX <= 4 ? 2 : 1;
#pragma unroll kStepUnroll
            for (int k = 0; k < N; ++k) {
                double K[NK], hFq[SQ], hFqd[FD], hFu[FU], Fk[NX], ck[NX], rk[NX], uk[NU];
#pragma unroll
                for (int i = 0; i < NK; ++i) K[i] = nK[i];
#pragma unroll
                for (int i = 0; i < FQ; ++i) hFq[i] = nFq[i];
#pragma unroll
                for (int i = 0; i < FD; ++i) hFqd[i] = nFqd[i];
#pragma unroll
                for (int i = 0; i < FU; ++i) hFu[i] = nFu[i];
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    Fk[r] = nF[r];
                    ck[r] = nc[r];
                    rk[r] = nr[r];
                }
#pragma unroll
                for (int c = 0; c < NU; ++c) uk[c] = nu_[c];
                if (k + 1 < N) GROUP_LOAD_STEP(k + 1);
                double du[NU];
#pragma unroll
                for (int a = 0; a < NU; ++a) {
                    double t = K[a * (NS + 1) + NS];
#pragma unroll
                    for (int q = 0; q < NX; ++q) t = fma(K[a * (NS + 1) + q], dx[q], t);
#pragma unroll
                    for (int c = 0; c < NU; ++c) t = fma(K[a * (NS + 1) + NX + c], dup[c], t);
                    du[a] = t;
                    sDU[k * NU + a] = t;
                }
                if (BOUNDED && pass + 1 < kBoundPasses) {  // a free control whose step crosses a bound: hold it
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        const double hv = sHold[k * NU + a], t = uk[a] + du[a];
                        if (hv != hv && (t < lbv[a] || t > ubv[a])) {
                            sHold[k * NU + a] = t < lbv[a] ? lbv[a] : ubv[a];
                            resolve = true;
                        }
                    }
                }
                double ad[NX];
                a_mul<NQ, NA, double>(h, hFq, hFqd, dx, ad);
#pragma unroll
                for (int s = 0; s < NA; ++s)
#pragma unroll
                    for (int c = 0; c < NU; ++c) ad[NQ + s] = fma(hFu[s * NU + c], du[c], ad[NQ + s]);
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    const double qe = 2.0 * Q[r] * (Fk[r] - rk[r]);
                    dJ = fma(qe, ad[r], dJ);
                    dx[r] = ad[r] + ck[r];
                    sDX[(k + 1) * NX + r] = dx[r];
                }
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    const double dif = uk[c] - um[c];
                    dJ = fma(2.0 * R[c] * dif, du[c] - dup[c], fma(2.0 * Rm[c] * uk[c], du[c], dJ));
                    um[c] = uk[c];
                    dup[c] = du[c];
                }
            }
#undef GROUP_LOAD_STEP
        };
