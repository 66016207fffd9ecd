// sqp_group_step.inc -- phase C of the lane-distributed path (kernel text, included once by sqp_group_body.inc inside
// its `if constexpr (DIST)`): the step sweep, Mehrotra's predictor-corrector block, the QP-pass / hold / release loop of
// the control-bounded solves and the directional derivative.
// expects: the spine's setup, load_arow (sqp_group_dist_grad.inc), backward_dist and backward_vec
//          (sqp_group_dist_riccati.inc), use_w, fact_ok, resolve, and the Riccati sweep's gains in wK / sKh.
// defines: step_dist(check) (local to the block); leaves the step in sDX | sDU, A dx + B du in sD, dJ; MEHR: mub = mu_t.
            // step sweep: lane r holds s_k[r], s = [dx_k; du_{k-1}]; u-lanes du_k = K_k s_k + kff_k (row r - NX of
            // K from the workspace), x-lanes dx_{k+1} = A dx + B du + c.  A dx_k + B du_k goes to sD[k+1] (d is
            // dead after the backward sweep) for the directional derivative below.
            // check: a free control whose step crosses a bound is held there (sHold) and the QP solved again (BOUNDED)
            auto step_dist = [&](bool check) {
                // K_k columns were stored by the other lanes of this wave in the backward sweep
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                constexpr bool RUN = MIRROR;   // running addresses, unmasked stores, no clamped prefetch (below)
                double sr = 0.0;
#if defined(MMPC_PHASE_TIMING) && defined(MMPC_PHASE_STAGES)
                if (gl == 0 && blockIdx.x < kPhaseWavePhases)
                    g_mmpc_phase_cycles[kPhaseStepLog + 8 * blockIdx.x + 2 * gi] = __builtin_amdgcn_s_memtime();
#endif
                if (RUN || lx) sDX[rx] = 0.0;
                constexpr int NK = NS + 1;
                const double* const Kp = wK + ru * NK;   // row ru of K_k | kff_k at Kp + k NU NK
                // the stage operands of a buffer: the K row from the HBM/L2 workspace, row r of [A - I | B] and c_k[r]
                // from LDS
                struct Ops {
                    double K[NK], a[NX], b[NU], c, Rw[BOUNDED ? NR : 1];
                };
                const double* const Rp = wRel + ru * NR;   // BOUNDED: un-held row ru at Rp + k NU NR
                // RUN: every address of the sweep runs along it, one add per stage, opaque to the loop optimiser -- the
                // lane's three row addresses and its c address (the stage of the next refill), the K (and un-held) row
                // pointer, and two store addresses:
                //   js: where the lane's s goes -- x-lanes dx_{k+1}[r] in sDX (stride NX), u-lanes du_k in sDU (stride NU);
                //       the stored value is the lane's next s, so one store serves both roles and s needs one select
                //   jt: where A dx_k + B du_k goes -- x-lanes sD[k+1][r] (stride NX).  A u-lane has no such row; its sum
                //       (finite: its own du_{k-1} plus row 0's products) goes to sD[ru] with stride 0.  sD[0 .. NX) is
                //       d_0: no sweep or pass of the lane-distributed kernels reads it (they start at sD[NX]), and the d
                //       recursion zeroes it again at the start of the next iteration.
                // A lane without a role carries lane 0's chain (rows, c and K row 0 as lane 0) and stores lane 0's
                // values to lane 0's addresses.
                using LdsW = __attribute__((address_space(3))) double*;
                [[maybe_unused]] LdsB ja = iAq, jd = iAd, jb = iBr, jcs = shb + 8 * ((int)(sC - shm) + rx);
                [[maybe_unused]] LdsB js = shb + 8 * (lu ? (int)(sDU - shm) + ru : (int)(sDX - shm) + NX + rx);
                [[maybe_unused]] LdsB jt = shb + 8 * (lu ? (int)(sD - shm) + ru : (int)(sD - shm) + NX + rx);
                [[maybe_unused]] const int zs = lu ? 8 * NU : 8 * NX, zt = lu ? 0 : 8 * NX;
                using GlbD = const __attribute__((address_space(1))) double*;   // (stays a global load behind the pin)
                [[maybe_unused]] GlbD jK = (GlbD)Kp;
                [[maybe_unused]] GlbD jR = (GlbD)Rp;
                // (hs: -1, or the stage 0 .. 2 whose K row the head block holds -- the opening's refills)
                [[maybe_unused]] auto refill = [&](Ops& o, int hs = -1) {   // the next stage in order
#pragma unroll
                    for (int j = 0; j < NK; ++j) o.K[j] = (KH > 0 && hs >= 0) ? sKh[(hs * NU + ru) * NK + j] : jK[j];
#pragma unroll
                    for (int s2 = 0; s2 < NQ; ++s2) o.a[s2] = lds(ja + 8 * s2);
#pragma unroll
                    for (int s2 = 0; s2 < NA; ++s2) o.a[NQ + s2] = lds(jd + 8 * s2);
#pragma unroll
                    for (int c = 0; c < NU; ++c) o.b[c] = lds(jb + 8 * c);
                    o.c = lds(jcs);
                    if constexpr (BOUNDED) {
#pragma unroll
                        for (int j = 0; j < NR; ++j) o.Rw[j] = jR[j];
                    }
                };
                [[maybe_unused]] auto advance = [&]() {
                    ja += zAq;
                    jd += zAd;
                    jb += zBr;
                    jcs += 8 * NX;
                    jK += NU * NK;
                    pin(ja);
                    pin(jd);
                    pin(jb);
                    pin(jcs);
                    asm volatile("" : "+v"(jK));
                    if constexpr (BOUNDED) {
                        jR += NU * NR;
                        asm volatile("" : "+v"(jR));
                    }
                };
                auto fetch = [&](int k, Ops& o) {
#pragma unroll
                    for (int j = 0; j < NK; ++j) o.K[j] = Kp[k * NU * NK + j];
                    load_arow(k, o.a, o.b);
                    o.c = sC[k * NX + rx];
                    if constexpr (BOUNDED) {
#pragma unroll
                        for (int j = 0; j < NR; ++j) o.Rw[j] = Rp[k * NU * NR + j];
                    }
                };
                // (more: RUN, whether the stage refills its buffer with the stage three ahead)
                auto stage = [&](int k, Ops& o, [[maybe_unused]] bool more = true) {
                    double sb[NS];
                    sfor<0, NS>([&](auto I) { sb[I] = row_bcast<I>(sr); });
                    double du0 = o.K[NS], du1 = 0.0;
#pragma unroll
                    for (int j = 0; j < NS; ++j) {
                        if (j & 1) du1 = fma(o.K[j], sb[j], du1);
                        else du0 = fma(o.K[j], sb[j], du0);
                    }
                    const double du = du0 + du1;
                    double ad = sr;
#pragma unroll
                    for (int j = 0; j < NX; ++j) ad = fma(o.a[j], sb[j], ad);
                    double dub[NU];
                    sfor<0, NU>([&](auto I) { dub[I] = row_bcast<NX + I>(du); });
#pragma unroll
                    for (int c = 0; c < NU; ++c) ad = fma(o.b[c], dub[c], ad);
                    const double dxn = ad + o.c;
                    if constexpr (RUN) {   // unmasked stores through the lane's running store addresses
                        sr = lu ? du : dxn;
                        *(LdsW)js = sr;
                        *(LdsW)jt = ad;
                        js += zs;
                        jt += zt;
                        pin(js);
                        pin(jt);
                    } else {
                        if (lx) {
                            sDX[(k + 1) * NX + rx] = dxn;
                            sD[(k + 1) * NX + rx] = ad;
                        }
                        if (lu) sDU[k * NU + ru] = du;
                    }
                    if constexpr (BOUNDED) {
                        if (check && lu) {
                            const double hv = sHold[k * NU + ru], t = sU[k * NU + ru] + du;
                            if (hv != hv) {   // free: hold it where its step crosses a bound
                                if (t < lbr || t > ubr) {
                                    sHold[k * NU + ru] = t < lbr ? lbr : ubr;
                                    resolve = true;
                                }
                            } else if (!p.no_release) {   // held: release it when its multiplier H_ww du + [H_wx | -R] s + h_w points inward
                                double m = o.Rw[NR - 1];
#pragma unroll
                                for (int j = 0; j < NS; ++j) m = fma(o.Rw[j], sb[j], m);
#pragma unroll
                                for (int b = 0; b < NU; ++b) m = fma(o.Rw[NS + b], dub[b], m);
                                if ((hv == lbr && m < 0.0) || (hv == ubr && m > 0.0)) {
                                    sHold[k * NU + ru] = NAN;
                                    resolve = true;
                                }
                            }
                        }
                    }
#if defined(MMPC_PHASE_TIMING) && defined(MMPC_PHASE_STAGES)
                    asm volatile("" ::"v"(sr), "v"(ad));
                    if (k == 0 && gl == 0 && blockIdx.x < kPhaseWavePhases)
                        g_mmpc_phase_cycles[kPhaseStepLog + 8 * blockIdx.x + 2 * gi + 1] = __builtin_amdgcn_s_memtime();
#endif
                    if constexpr (RUN) {
                        if (more) {
                            refill(o);
                            advance();
                        }
                    } else {
                        sr = lx ? dxn : (lu ? du : 0.0);
                        fetch(k + 3 < N ? k + 3 : N - 1, o);   // unconditional: static wait counts
                    }
                };
                // three buffers, refilled three stages ahead: the K rows come from L2/MALL (the workspace of a
                // 512-instance XCD exceeds its 4 MB L2) and one stage of the sweep (~300 cycles) did not cover that
                // latency -- with two buffers every stage waited for the loads issued one stage earlier
                Ops o0, o1, o2;
                if constexpr (RUN) {
                    // No clamp and no read past stage N - 1.  The N - 3 stages that have a stage three ahead refill their
                    // buffer: the three-stage body takes them three at a time (the same outstanding loads on every path
                    // at its top: the wait before stage k's operands is vmcnt(#loads of stages k + 1, k + 2)), the one
                    // or two left over follow it; the last three stages run without a refill, from the buffers the
                    // rotation has reached.  The opening loads of a horizon shorter than three read its last stage
                    // again (values never used) instead of moving on.
                    // With the head block (KH) the opening's K rows are LDS reads, under one uniform test for the
                    // horizons that have three stages (the form with a test between the refills makes the exact kernel
                    // spill two registers); the K pointer runs along, so that the first refill of a stage finds row 3
                    // of the workspace.  Where the K rows come from the workspace the test sits between the refills:
                    // the uniform form measured slower there (DESIGN.md 4c, round 23).
                    if (KH == 0 || N < 3) {
                        refill(o0, 0);
                        if (N > 1) advance();
                        refill(o1, N > 1 ? 1 : 0);
                        if (N > 2) advance();
                        refill(o2, N > 2 ? 2 : N - 1);
                        advance();
                    } else {
                        refill(o0, 0);
                        advance();
                        refill(o1, 1);
                        advance();
                        refill(o2, 2);
                        advance();
                    }
                    int k = 0;
                    for (; k + 5 < N; k += 3) {
                        stage(k, o0, true);
                        stage(k + 1, o1, true);
                        stage(k + 2, o2, true);
                    }
                    const int left = N - 3 - k;   // refilling stages left: 0, 1 or 2 (negative: N < 3)
                    if (left == 1) {
                        stage(k, o0, true);
                        stage(k + 1, o1, false);
                        stage(k + 2, o2, false);
                        stage(k + 3, o0, false);
                    } else if (left == 2) {
                        stage(k, o0, true);
                        stage(k + 1, o1, true);
                        stage(k + 2, o2, false);
                        stage(k + 3, o0, false);
                        stage(k + 4, o1, false);
                    } else {
                        stage(k, o0, false);
                        if (N >= 2) stage(k + 1, o1, false);
                        if (N >= 3) stage(k + 2, o2, false);
                    }
                    return;
                }
                // (the other models: the clamped prefetch, N mod 3 stages peeled in front)
                fetch(0, o0);
                fetch(N > 1 ? 1 : 0, o1);
                fetch(N > 2 ? 2 : 0, o2);
                // all three stages of the unrolled body unconditional (N mod 3 stages peeled in front, the buffers
                // rotate roles): the loop top then has the same outstanding loads on every path, so the wait before
                // stage k's operands is vmcnt(#loads of stages k+1, k+2), not vmcnt(0)
                if (N % 3 == 1) {
                    stage(0, o0);
                    for (int k = 1; k < N; k += 3) {
                        stage(k, o1);
                        stage(k + 1, o2);
                        stage(k + 2, o0);
                    }
                } else if (N % 3 == 2) {
                    stage(0, o0);
                    stage(1, o1);
                    for (int k = 2; k < N; k += 3) {
                        stage(k, o2);
                        stage(k + 1, o0);
                        stage(k + 2, o1);
                    }
                } else {
                    for (int k = 0; k < N; k += 3) {
                        stage(k, o0);
                        stage(k + 1, o1);
                        stage(k + 2, o2);
                    }
                }
            };
            if constexpr (MEHR) {
                // affine predictor step (the sweep above ran with b = 0): dy_aff in sDX | sDU
                step_dist(false);
                __builtin_amdgcn_wave_barrier();
                // stage-parallel: steps to the boundary without tau, mu = avg(s z), mu_aff at the end of those steps
                double ap = 1.0, ad = 1.0, sz = 0.0;
                for (int k = gl; k < N; k += G) {
#pragma unroll
                    for (int j = 0; j < NS; ++j) {
                        const double y = j < NX ? sX[(k + 1) * NX + j] : sU[k * NU + j - NX];
                        const double dy = j < NX ? sDX[(k + 1) * NX + j] : sDU[k * NU + j - NX];
                        ip_aff_limits(y, dy, yl[j], yu[j], sZl[k * NS + j], sZu[k * NS + j], ap, ad, sz);
                    }
                }
                ap = group_min(ap);
                ad = group_min(ad);
                sz = group_sum(sz);
                double saff = 0.0;
                for (int k = gl; k < N; k += G) {
#pragma unroll
                    for (int j = 0; j < NS; ++j) {
                        const double y = j < NX ? sX[(k + 1) * NX + j] : sU[k * NU + j - NX];
                        const double dy = j < NX ? sDX[(k + 1) * NX + j] : sDU[k * NU + j - NX];
                        saff += ip_aff_compl(y, dy, yl[j], yu[j], sZl[k * NS + j], sZu[k * NS + j], ap, ad);
                    }
                }
                saff = group_sum(saff);
                int nb = 0;   // finite bounds of one stage
#pragma unroll
                for (int j = 0; j < NS; ++j) nb += (yl[j] > -INFINITY) + (yu[j] < INFINITY);
                const double mbnd = (double)nb * (double)N;
                const double muc = sz / mbnd, mua = saff / mbnd;   // XB: at least one finite bound
                const double sig = muc > 0.0 ? pow(mua / muc, 3.0) : 0.0;
                // the target mu_t replaces the barrier parameter of this iteration (merit, duals, safeguard, trace)
                mub = fmax(kIpTolCompl / 20.0, fmin(sig * muc, kIpMu0));
                for (int k = gl; k < N; k += G) {
#pragma unroll
                    for (int j = 0; j < NS; ++j) {
                        const double y = j < NX ? sX[(k + 1) * NX + j] : sU[k * NU + j - NX];
                        const double dy = j < NX ? sDX[(k + 1) * NX + j] : sDU[k * NU + j - NX];
                        double ccl, ccu, bb;
                        ip_corrector(y, dy, yl[j], yu[j], sZl[k * NS + j], sZu[k * NS + j], mub, ccl, ccu, bb);
                        sCl[k * NS + j] = ccl;
                        sCu[k * NS + j] = ccu;
                        sBb[k * NS + j] = bb;
                    }
                }
                // the corrected b of every stage visible to the other lanes' sweep
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                // corrector: the same stage matrices and factors with the corrected b -- only the vector part of the
                // recursion changes (backward_vec); the usual step sweep follows
                backward_vec();
            }
            for (int pass = 0;; ++pass) {
                if (pass > 0) {   // BOUNDED: controls held after the previous step -- solve the QP again
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    backward_dist(use_w);
                    if (EXACT && use_w && !fact_ok) {   // the held exact QP not positive definite: Gauss-Newton
                        fact_ok = 1;
                        use_w = false;
                        backward_dist(false);
                    }
                    if (!fact_ok) break;
                }
                resolve = false;
                // QP solves of this iteration: two at the first (the cold start's active set moves most there, and a
                // wave pays its slowest instance's solves), kBoundPasses later (oracle bound_release)
                const int passes = (it == 0 && !p.no_release) ? 2 : kBoundPasses;
                step_dist(BOUNDED && pass + 1 < passes);
                if constexpr (!BOUNDED) {
                    break;
                } else {
                    resolve = group_max(resolve ? 1.0 : 0.0) != 0.0;
                    if (!resolve || pass + 1 >= passes) break;
                }
            }
            __builtin_amdgcn_wave_barrier();
            // directional derivative of J along (dx, du), stage-parallel:
            // sum_k 2Q(F_k - r_k).(A dx_k + B du_k) + 2R(u_k - u_{k-1})(du_k - du_{k-1}) + 2Rm u_k du_k
            double dj = 0.0;
            for (int k0 = gl; k0 < N; k0 += WD * G) {   // (PAIR: the loads of two stages in flight together)
                double ef[WD][NX], ad[WD][NX], uk[WD][NU], duk[WD][NU], um[WD][NU], dum[WD][NU];
#pragma unroll
                for (int e = 0; e < WD; ++e) {
                    const int k = (e == 0 || k0 + e * G < N) ? k0 + e * G : k0;
#pragma unroll
                    for (int q = 0; q < NX; ++q) {
                        ef[e][q] = sF[k * NX + q] - tr[k * NX + q];
                        ad[e][q] = sD[(k + 1) * NX + q];
                    }
#pragma unroll
                    for (int c = 0; c < NU; ++c) {
                        uk[e][c] = sU[k * NU + c];
                        duk[e][c] = sDU[k * NU + c];
                        um[e][c] = (k == 0) ? up[c] : sU[(k - 1) * NU + c];
                        dum[e][c] = (k == 0) ? 0.0 : sDU[(k - 1) * NU + c];
                    }
                }
#pragma unroll
                for (int e = 0; e < WD; ++e) {
                    double ds = dj;
#pragma unroll
                    for (int q = 0; q < NX; ++q) ds = fma(2.0 * Q[q] * ef[e][q], ad[e][q], ds);
#pragma unroll
                    for (int c = 0; c < NU; ++c)
                        ds = fma(2.0 * R[c] * (uk[e][c] - um[e][c]), duk[e][c] - dum[e][c], fma(2.0 * Rm[c] * uk[e][c], duk[e][c], ds));
                    dj = (e == 0 || k0 + e * G < N) ? ds : dj;
                }
            }
            dJ = group_sum(dj);
