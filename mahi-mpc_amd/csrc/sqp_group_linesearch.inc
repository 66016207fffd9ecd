// sqp_group_linesearch.inc -- phase D of an iteration of the 16-lane kernel (kernel text, included once by
// sqp_group_body.inc at the end of its iteration loop): the interior point's step limits, the l1-merit line search with
// its fused first trial, and the update of the iterate and the duals.
// expects: the spine's setup, J0, c1, lsum, cmpl0 (phase A), lmax, dJ, mub_next, trc, and the step in sDX | sDU.
// defines: trial; sets mu, mub, fwd_ready and the hand-over J0n, c1n, cmaxn, nfn; leaves the loop with ST_LS_FAILED.
        // interior point: fraction to the boundary (primal alpha_max, dual alpha_z), barrier directional derivative
        double amax = 1.0, az = 1.0, dbar = 0.0;
        if constexpr (XB) {
            const double tau = kIpTau;
            for (int k = gl; k < N; k += G) {
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    const double y = j < NX ? sX[(k + 1) * NX + j] : sU[k * NU + j - NX];
                    const double dy = j < NX ? sDX[(k + 1) * NX + j] : sDU[k * NU + j - NX];
                    if constexpr (MEHR)
                        ip_step_limits_pc(y, dy, yl[j], yu[j], sZl[k * NS + j], sZu[k * NS + j], mub, tau,
                                          sCl[k * NS + j], sCu[k * NS + j], amax, az, dbar);
                    else
                        ip_step_limits(y, dy, yl[j], yu[j], sZl[k * NS + j], sZu[k * NS + j], mub, tau, sBb[k * NS + j],
                                       amax, az, dbar);
                }
            }
            amax = group_min(amax);
            az = group_min(az);
            dbar = group_sum(dbar);
        }

        // ---- D. stage-parallel l1-merit Armijo line search (noise-aware, as sqp_wave.h), update ----
        mu = fmax(mu, 4.0 * lmax + 1.0);
        const double phi0 = XB ? fma(mu, c1, fma(-2.0 * mub, lsum, J0)) : fma(mu, c1, J0);
        const double dphi = XB ? dJ + dbar - mu * c1 : dJ - mu * c1;
        double alpha = amax;
        bool accepted = false;
        // The fused forward pass: the line search's alpha = 1 trial evaluates the model with its Jacobian and writes
        // everything phase A computes at that point (F_k, c_k, the stage blocks; J, |c|_1, max|c|); when the full step is
        // accepted (every cfg#2 iteration, tools/alpha_stats.py) the next iteration skips phase A.  The trial point
        // fma(1, d, v) is the update's iterate and the sums run in phase A's order, so the values are phase A's bit for bit.
        // The old stage blocks are dead once the directional derivative is formed; a rejected full step recomputes them in
        // phase A.
        // XB (round 5): the first trial is at alpha = alpha_max (fraction to the boundary) and the update's y is the same
        // fma(alpha, dy, y) (ip_update), so the fused evaluation is again phase A's; the barrier terms (ip_terms) of phase
        // A still run every iteration, after the dual update.
        // ctm, nft are phase A's max|c| and nonfinite flag at that trial
        double ctm = 0.0;
        int nft = 0;
        auto trial = [&](auto jac_c, double& Jt, double& ct, double& lt) {
            constexpr bool JAC = decltype(jac_c)::value;
            // two stages per lane in the fused trial; the trials after a rejected full step keep the one-stage loop (no
            // cfg#2 iteration runs them, and with nothing to store the compiler puts a pair's second evaluation behind a
            // branch on "the lane has a second stage" anyway)
            constexpr int WT = JAC ? WD : 1;
            with_lin(std::integral_constant<int, WT>{}, [&](auto lm_c) {
                constexpr int LM = decltype(lm_c)::value;
                for (int k0 = gl; k0 < N; k0 += WT * G) {
                    int kk[WT];
                    double x[WT][NX], u[WT][NU], xd[WT][NX];
                    [[maybe_unused]] double Fq[WT][SQ], Fqd[WT][FD], Fu[WT][FU];
#pragma unroll
                    for (int e = 0; e < WT; ++e) {
                        const int k = kk[e] = (e == 0 || k0 + e * G < N) ? k0 + e * G : k0;
#pragma unroll
                        for (int r = 0; r < NX; ++r) x[e][r] = fma(alpha, sDX[k * NX + r], sX[k * NX + r]);
#pragma unroll
                        for (int c = 0; c < NU; ++c) {
                            u[e][c] = fma(alpha, sDU[k * NU + c], sU[k * NU + c]);
                            if (BOUNDED) u[e][c] = proj(u[e][c], lbv[c], ubv[c]);  // projected trial point
                        }
                    }
                    group_model_w<Model, WT, LM, JAC, SQ, FD, FU>(lin, lFq, lFqd, lFu, lxd, lxs, up, x, u, xd, Fq, Fqd, Fu);
                    double cd[WT][NX], er[WT][NX];
#pragma unroll
                    for (int e = 0; e < WT; ++e) {
                        const int k = kk[e];
                        if constexpr (JAC) {   // = phase A at the trial point (stored for the next iteration)
#pragma unroll
                            for (int i = 0; i < FQ; ++i) sFq[k * FQ + i] = h * Fq[e][i];
#pragma unroll
                            for (int i = 0; i < FD; ++i) sFqd[k * FD + i] = h * Fqd[e][i];
#pragma unroll
                            for (int i = 0; i < FU; ++i) sFu[k * FU + i] = h * Fu[e][i];
                        }
#pragma unroll
                        for (int r = 0; r < NX; ++r) {
                            const double F = fma(h, xd[e][r], x[e][r]);
                            if constexpr (JAC) sF[k * NX + r] = F;
                            if constexpr (JAC) {
                                cd[e][r] = F - fma(alpha, sDX[(k + 1) * NX + r], sX[(k + 1) * NX + r]);
                                sC[k * NX + r] = cd[e][r];
                                er[e][r] = F - tr[k * NX + r];
                            } else {
                                er[e][r] = F - tr[k * NX + r];
                                cd[e][r] = F - fma(alpha, sDX[(k + 1) * NX + r], sX[(k + 1) * NX + r]);
                            }
                        }
                    }
                    // the sums in stage order; a repeated stage leaves them as they were
#pragma unroll
                    for (int e = 0; e < WT; ++e) {
                        const int k = kk[e];
                        double Js = Jt, cs = ct, ls = lt;
#pragma unroll
                        for (int r = 0; r < NX; ++r) {
                            if constexpr (JAC) {
                                ctm = fmax(ctm, fabs(cd[e][r]));
                                cs += fabs(cd[e][r]);
                                nft |= !isfinite(cd[e][r]);
                                Js = fma(er[e][r] * Q[r], er[e][r], Js);
                            } else {
                                Js = fma(er[e][r] * Q[r], er[e][r], Js);
                                cs += fabs(cd[e][r]);
                            }
                        }
#pragma unroll
                        for (int c = 0; c < NU; ++c) {
                            double um = (k == 0) ? up[c] : fma(alpha, sDU[(k - 1) * NU + c], sU[(k - 1) * NU + c]);
                            if (BOUNDED && k > 0) um = proj(um, lbv[c], ubv[c]);
                            const double dif = u[e][c] - um;
                            Js = fma(dif * R[c], dif, fma(u[e][c] * Rm[c], u[e][c], Js));
                        }
                        if constexpr (XB) {
#pragma unroll
                            for (int j = 0; j < NS; ++j) {
                                const double y = j < NX ? fma(alpha, sDX[(k + 1) * NX + j], sX[(k + 1) * NX + j]) : u[e][j - NX];
                                ls += ip_log_slacks(y, yl[j], yu[j]);
                            }
                        }
                        const bool on = e == 0 || k0 + e * G < N;
                        Jt = on ? Js : Jt;
                        ct = on ? cs : ct;
                        lt = on ? ls : lt;
                    }
                }
            });
        };
        bool jac_trial = false;
        const FirstIterSwitch fsw = first_iter_switch(!XB && it == 0, c1, dJ);
        for (int ls = 0; ls < 30; ++ls) {
            double Jt = 0.0, ct = 0.0, lt = 0.0;
            jac_trial = ls == 0;   // alpha = amax (1 without state bounds)
            if (jac_trial) trial(std::true_type{}, Jt, ct, lt);
            else trial(std::false_type{}, Jt, ct, lt);
            Jt = group_sum(Jt);
            ct = group_sum(ct);
            if (XB) lt = group_sum(lt);
            const double phit = XB ? fma(mu, ct, fma(-2.0 * mub, lt, Jt)) : fma(mu, ct, Jt);
            const double noise = 1.0 + fabs(phi0);
            if (dphi >= -1e-11 * noise || phit <= phi0 + 1e-4 * alpha * dphi + 1e-13 * noise ||
                (!XB && it == 0 && first_iter_filter_accepts(J0, c1, Jt, ct, alpha, fsw))) {
                accepted = true;
                if (jac_trial) {   // the next iteration starts after phase A
                    fwd_ready = true;
                    J0n = Jt;
                    c1n = ct;
                    cmaxn = group_max(ctm);
                    nfn = nft;
                }
                break;
            }
            alpha *= 0.5;
        }
        if (trc && gl == 0) {
            trc[4] = XB ? amax : dJ;
            trc[5] = alpha;
            trc[6] = XB ? mub : mu;
            if (XB) trc[3] = cmpl0;
        }
        MMPC_PHASE(5);
        if (!accepted) {
            status = ST_LS_FAILED;
            break;
        }
        __builtin_amdgcn_wave_barrier();
        if constexpr (XB) {  // y and the duals of stage k's (x_{k+1} | u_k), as oracle solve_one_ip
            for (int k = gl; k < N; k += G) {
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    double& y = j < NX ? sX[(k + 1) * NX + j] : sU[k * NU + j - NX];
                    const double dy = j < NX ? sDX[(k + 1) * NX + j] : sDU[k * NU + j - NX];
                    double zl = sZl[k * NS + j], zu = sZu[k * NS + j], yn;
                    if constexpr (MEHR)
                        ip_update_pc(y, dy, yl[j], yu[j], zl, zu, mub, sCl[k * NS + j], sCu[k * NS + j], alpha, az, yn);
                    else
                        ip_update(y, dy, yl[j], yu[j], zl, zu, mub, alpha, az, yn);
                    y = yn;
                    sZl[k * NS + j] = zl;
                    sZu[k * NS + j] = zu;
                }
            }
            if constexpr (!MEHR) mub = mub_next;   // MEHR: no lagged update, mu_t is set in every iteration
        } else {
            // (PAIR: all loads of the two stages before their stores -- a repeated stage forms its new value from the old
            // one both times and stores it twice)
            for (int k0 = gl; k0 <= N; k0 += WD * G) {
                int kk[WD], ku[WD];
                double xn[WD][NX], un[WD][NU];
#pragma unroll
                for (int e = 0; e < WD; ++e) {
                    const int k = kk[e] = (e == 0 || k0 + e * G <= N) ? k0 + e * G : k0;
                    if constexpr (WD == 1) {
                        ku[e] = k;
                        if (k > 0) {
#pragma unroll
                            for (int r = 0; r < NX; ++r) xn[e][r] = fma(alpha, sDX[k * NX + r], sX[k * NX + r]);
                        }
                        if (k < N) {
#pragma unroll
                            for (int c = 0; c < NU; ++c) un[e][c] = fma(alpha, sDU[k * NU + c], sU[k * NU + c]);
                        }
                    } else {   // loads without lane tests: x_0 keeps its bytes by a select, k = N reads the u row of N - 1
                        ku[e] = k < N ? k : N - 1;
#pragma unroll
                        for (int r = 0; r < NX; ++r) {
                            const double xo = sX[k * NX + r];
                            xn[e][r] = k > 0 ? fma(alpha, sDX[k * NX + r], xo) : xo;
                        }
#pragma unroll
                        for (int c = 0; c < NU; ++c) un[e][c] = fma(alpha, sDU[ku[e] * NU + c], sU[ku[e] * NU + c]);
                    }
                }
                if constexpr (WD > 1) __builtin_amdgcn_wave_barrier();   // (compiler: no store of the pair above a load)
#pragma unroll
                for (int e = 0; e < WD; ++e) {
                    const int k = kk[e];
                    if (WD > 1 || k > 0) {
#pragma unroll
                        for (int r = 0; r < NX; ++r) sX[k * NX + r] = xn[e][r];
                    }
                    if (k < N) {   // (never the u row of another lane's stage: that lane updates it itself)
#pragma unroll
                        for (int c = 0; c < NU; ++c) sU[ku[e] * NU + c] = BOUNDED ? proj(un[e][c], lbv[c], ubv[c]) : un[e][c];
                    }
                }
            }
        }
