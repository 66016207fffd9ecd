// sqp_group_dist_grad.inc -- the lane-distributed sweeps in front of the stop test (kernel text, included once by
// sqp_group_body.inc): the d recursion, the adjoint and the reduced gradient, and the row / column loads of A_k that all
// lane-distributed sweeps share.  DIST kernels run them; the others compile them unused.
// expects: the spine's setup (lane roles, per-lane operand addresses iAq .. iAcN, lds, pin) and, of this iteration,
//          nonfinite, gmax, lmax, beps.
// defines: colA, load_arow, d_recursion_dist, load_acol, adjoint_dist.
        // ---- DIST: the same recursions with row r of every quantity on lane r of the group ----
        // column r of A (x-lanes): own row (identity) + h in row z for r = NQ + z + acol[t] in row NQ + t, where
        // acol = hFq[:, r] (q-lanes) or hFqd[:, r - NQ] (a-lanes); so (A^T v)[r] = colA(v_r, vb) with vb = all v.
        auto colA = [&](double own, const double* acol, const double* vb) {
            double t = lxf * own;
#pragma unroll
            for (int z = 0; z < NQ; ++z) t = fma(hq[z], vb[z], t);
#pragma unroll
            for (int s2 = 0; s2 < NA; ++s2) t = fma(acol[s2], vb[NQ + s2], t);
            return t;
        };
        // row r of [A - I | B] (x-lanes) at stage k: q-lanes h e_{NQ+r}, a-lanes [hFq, hFqd | hFu] row r - NQ
        // (unconditional loads through the lane's own index and stage stride, iAq / iAd / iBr above: a conditional LDS
        // load becomes a branch, and a select between a loaded value and a register a flat load through a selected
        // LDS-or-scratch pointer)
        auto load_arow = [&](int k, double* arow, double* brow) {
#pragma unroll
            for (int s2 = 0; s2 < NQ; ++s2)
                arow[s2] = LOPS ? lds(iAq + __mul24(k, zAq) + 8 * s2) : fma(lad, sFq[k * FQ + ta * NQ + s2], hrow[s2]);
#pragma unroll
            for (int s2 = 0; s2 < NA; ++s2)
                arow[NQ + s2] = LOPS ? lds(iAd + __mul24(k, zAd) + 8 * s2) : fma(lad, sFqd[k * FD + ta * NA + s2], hrow[NQ + s2]);
#pragma unroll
            for (int c = 0; c < NU; ++c) brow[c] = LOPS ? lds(iBr + __mul24(k, zBr) + 8 * c) : lad * sFu[k * FU + ta * NU + c];
        };
        // d_{k+1} = A_k d_k + c_k (d_0 = 0): lane r holds d_k[r]
        // The recursions below are latency-bound (a few FMAs per stage on the dependency chain): every stage's
        // LDS operands are loaded one stage ahead and the dot products split into two partial sums.
        auto d_recursion_dist = [&]() {
            double dr = 0.0;
            if (MIRROR || lx) sD[rx] = 0.0;   // (also what re-zeroes the step sweep's dump doubles, see step_dist)
            // stage operands (row r of A - I through the lane's own address, used as loaded; the wait for a load sits a
            // full stage after its issue): two buffers, each refilled two stages ahead.  MIRROR: a buffer is refilled
            // after its last use in program order (the refill closes the stage, behind a scheduling barrier), so the
            // old and the new contents are never live together and the unroll by two renames the buffers without a copy.
            struct Op {
                double q[NQ > 0 ? NQ : 1], d[NA], c;
            };
            // (the lane's two row addresses run along with the fetches, one add each per stage: fetch k is the k-th call)
            LdsB jq = iAq, jd = iAd;
            auto fetch = [&](int k, Op& o) {
#pragma unroll
                for (int s2 = 0; s2 < NQ; ++s2) o.q[s2] = LOPS ? lds(jq + 8 * s2) : sFq[k * FQ + ta * NQ + s2];
#pragma unroll
                for (int s2 = 0; s2 < NA; ++s2) o.d[s2] = LOPS ? lds(jd + 8 * s2) : sFqd[k * FD + ta * NA + s2];
                o.c = sC[k * NX + rx];
                if constexpr (LOPS) {
                    jq += zAq;
                    jd += zAd;
                    pin(jq);
                    pin(jd);
                }
            };
            auto stage = [&](int k, Op& o) {
                double db[NX], arow[NX];
#pragma unroll
                for (int s2 = 0; s2 < NQ; ++s2) arow[s2] = LOPS ? o.q[s2] : fma(lad, o.q[s2], hrow[s2]);
#pragma unroll
                for (int s2 = 0; s2 < NA; ++s2) arow[NQ + s2] = LOPS ? o.d[s2] : fma(lad, o.d[s2], hrow[NQ + s2]);
                const double cr = o.c;
                // unconditional and unclamped (static wait counts; the address is a strength-reduced increment): past
                // the last stage the loads read the next arrays of this instance's LDS block (sFq -> sFqd -> sFu,
                // sC -> sFq), values never used
                if constexpr (!MIRROR) fetch(k + 2, o);
                sfor<0, NX>([&](auto I) { db[I] = row_bcast<I>(dr); });
                double t0 = dr + cr, t1 = 0.0;
#pragma unroll
                for (int j = 0; j < NX; ++j) {
                    if (j & 1) t1 = fma(arow[j], db[j], t1);
                    else t0 = fma(arow[j], db[j], t0);
                }
                // no lane-role mask on the chain: only the x-lanes' d is broadcast.  MIRROR: the other lanes carry lane 0's
                // d and store it again over lane 0's (same address, same bits), so the store needs no exec mask;
                // otherwise their finite leftovers (a sum of c_k[0]) are never read or stored
                dr = t0 + t1;
                if (MIRROR || lx) sD[(k + 1) * NX + rx] = dr;
                if constexpr (MIRROR) {
                    __builtin_amdgcn_sched_barrier(0);   // the refill stays behind the last use of o
                    fetch(k + 2, o);
                }
            };
            Op o0, o1;
            fetch(0, o0);
            fetch(LOPS || N > 1 ? 1 : 0, o1);   // LOPS: the second call, stage 1 (N = 1: stage N, as the prefetches below)
            int k = 0;
            for (; k + 1 < N; k += 2) {
                stage(k, o0);
                stage(k + 1, o1);
            }
            if (k < N) stage(k, o0);
        };
        // adjoint + reduced gradient + Riccati backward sweep; lane r: row r of P~ (Prow) and p~ (pvr), lam[r]
        // column r of the a-rows of A at stage k: hFq[:, r] (q-lanes), hFqd[:, r - NQ] (a-lanes), 0 otherwise
        // (ACOLP: jc = the lane's column address at stage k, kept by the caller, which takes the stages N - 1 .. 0 in order:
        // it leaves here one stage down, one add per stage)
        auto load_acol = [&](int k, [[maybe_unused]] LdsB& jc, double* acol) {
            if constexpr (ACOLP) {
#pragma unroll
                for (int t2 = 0; t2 < NA; ++t2) acol[t2] = lds(jc + 8 * t2 * NA);
                jc -= zAc;
                pin(jc);
            } else {
#pragma unroll
                for (int t2 = 0; t2 < NA; ++t2) {
                    double v = lad * sFqd[k * FD + t2 * NA + ta];
                    if constexpr (NQ > 0) v = fma(lqd, sFq[k * FQ + t2 * NQ + rq], v);
                    acol[t2] = v;
                }
            }
        };
        // adjoint lam_k = Q e_{k-1} + A_k^T lam_{k+1} (lam_N = Q e_{N-1}, e_{k-1} = d_k + x_k - r_{k-1}), lane r holds
        // lam[r] (x-lanes) and writes it over d_k in sD (d_k is read one stage earlier); then, stage-parallel, the
        // reduced gradient g_k = B_k^T lam_{k+1} + R (u_k - u_{k-1}) + Rm u_k - R (u_{k+1} - u_k) from the stored
        // lam (the serial sweep carries only the lam chain: the gradient's loads and arithmetic were a quarter of
        // its instructions).  gmax, lmax are per-lane maxima (reduced by the caller).
        // Runs before the stop test, so a converged wave skips the Riccati sweep.
        auto adjoint_dist = [&]() {
            double lamr;
            // MIRROR: a lane without an x row carries lane 0's lam (Q, column, operands and stores of row 0), so the
            // stores need no exec mask and lmax no lane factor (the maximum over the group sees lane 0's value twice);
            // Qa is the Q of the row the lane carries (without MIRROR: Qr)
            {
                const double eb = (MIRROR || lx) ? sX[N * NX + rx] - tr[(N - 1) * NX + rx] : 0.0;   // x_N - r_{N-1}
                lamr = Qa * (sD[N * NX + rx] + eb);
                if constexpr (XB) lamr += (MIRROR ? 1.0 : lxf) * sZg[(N - 1) * NS + rx];   // z_u - z_l of x_N's bounds
                lmax = fmax(lmax, fabs(lamr));
                if (MIRROR || lx) sD[N * NX + rx] = lamr;   // lam_k replaces d_k (read one stage earlier)
            }
            // stage operands as loaded, two buffers refilled two stages ahead (d_k is read before stage k writes lam_k
            // over it): column r of A's a-rows and the pieces of Q (d_k + x_k - r_{k-1})[r], combined at the use
            struct Op {
                double fd[NA], fq[NA], xk, trm, dk, zg;
            };
            // ACOLP: the lane's column address runs down with the fetches, one add per stage and no clamp: fetch number
            // i reads stage N - 1 - i, and the two fetches past stage 1 (values never used) read stages 0 and -1 of the
            // lane's array -- the end of the array in front of it (sC, sFq), inside the instance's block
            [[maybe_unused]] LdsB jc = (!MIRROR || lx) ? iAcN : shb + 8 * ((int)(sFq - shm) + (N - 1) * FD);
            [[maybe_unused]] const int zc = MIRROR ? 8 * FD : zAc;   // (every x-lane is a q- or an a-lane)
            auto fetch = [&](int k, Op& o) {   // k >= 1
#pragma unroll
                for (int t2 = 0; t2 < NA; ++t2) {
                    if constexpr (ACOLP) {
                        o.fd[t2] = lds(jc + 8 * t2 * NA);
                    } else {
                        o.fd[t2] = sFqd[k * FD + t2 * NA + ta];
                        if constexpr (NQ > 0) o.fq[t2] = sFq[k * FQ + t2 * NQ + rq];
                    }
                }
                if constexpr (ACOLP) {
                    jc -= zc;
                    pin(jc);
                }
                o.xk = sX[k * NX + rx];
                o.trm = tr[(k - 1) * NX + rx];
                o.dk = sD[k * NX + rx];
                if constexpr (XB) o.zg = sZg[(k - 1) * NS + rx];   // z_u - z_l of x_k's bounds
            };
            // stage k >= 1: lam_k from lam_{k+1}; then refill o with stage k - 2 (k >= 3; MIRROR: where `more` says so)
            auto stage = [&](int k, Op& o, [[maybe_unused]] bool more = true) {
                double acol[NA];
#pragma unroll
                for (int t2 = 0; t2 < NA; ++t2) {
                    if constexpr (ACOLP) {
                        acol[t2] = o.fd[t2];
                    } else {
                        double v = lad * o.fd[t2];
                        if constexpr (NQ > 0) v = fma(lqd, o.fq[t2], v);
                        acol[t2] = v;
                    }
                }
                double qe = Qa * (o.dk + (o.xk - o.trm));
                if constexpr (XB) qe += o.zg;
                if constexpr (!MIRROR) fetch(k >= 3 ? k - 2 : 1, o);   // unconditional: static wait counts
                double lamb[NX];
                sfor<0, NX>([&](auto I) { lamb[I] = row_bcast<I>(lamr); });
                // (A^T lam)[r] + Q e_{k-1}[r], two partial sums
                // unmasked chain: a lane without an x row carries lane 0's lam (MIRROR), stored again over lane 0's;
                // otherwise it has Qr = 0, acol = 0 and hq = 0, so it carries 0 (XB: a finite sum of another row's z
                // gaps) -- never broadcast or stored, and masked out of lmax
                double t0 = lamr + qe, t1 = 0.0;
#pragma unroll
                for (int z = 0; z < NQ; ++z) t1 = fma(hq[z], lamb[z], t1);
#pragma unroll
                for (int s2 = 0; s2 < NA; ++s2) {
                    if (s2 & 1) t1 = fma(acol[s2], lamb[NQ + s2], t1);
                    else t0 = fma(acol[s2], lamb[NQ + s2], t0);
                }
                lamr = t0 + t1;
                lmax = fmax(lmax, fabs(MIRROR ? lamr : lxf * lamr));
                if (MIRROR || lx) sD[k * NX + rx] = lamr;
                if constexpr (MIRROR) {   // the refill closes the stage, behind the last use of o (no buffer copies)
                    __builtin_amdgcn_sched_barrier(0);
                    if (more) fetch(k - 2, o);
                }
            };
            if (N >= 2) {
                Op o0, o1;
                fetch(N - 1, o0);
                fetch(N >= 3 ? N - 2 : 1, o1);
                int k = N - 1;
                if constexpr (MIRROR) {
                    // no clamp: the pair loop takes the stages whose refills (k - 2, k - 3) exist, unconditionally
                    // (static wait counts at its top); the two or three stages left run apart, stage 3 with its refill
                    for (; k >= 4; k -= 2) {
                        stage(k, o0);
                        stage(k - 1, o1);
                    }
                    if (k == 3) {
                        stage(3, o0);
                        stage(2, o1, false);
                        stage(1, o0, false);
                    } else if (k == 2) {
                        stage(2, o0, false);
                        stage(1, o1, false);
                    } else {
                        stage(1, o0, false);
                    }
                } else {
                    for (; k >= 2; k -= 2) {
                        stage(k, o0);
                        stage(k - 1, o1);
                    }
                    if (k == 1) stage(1, o0);
                }
            }
            // the lam rows of the other lanes of this wave must be visible to the gradient pass
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            for (int k = gl; k < N; k += G) {
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    double g = 0.0;
#pragma unroll
                    for (int s2 = 0; s2 < NA; ++s2) g = fma(sFu[k * FU + s2 * NU + c], sD[(k + 1) * NX + NQ + s2], g);
                    const double uk = sU[k * NU + c], um = k == 0 ? up[c] : sU[(k - 1) * NU + c];
                    g = fma(R[c], uk - um, fma(Rm[c], uk, g));
                    if (k < N - 1) g -= R[c] * (sU[(k + 1) * NU + c] - uk);
                    if constexpr (XB) g += sZg[k * NS + NX + c];   // reduced Lagrangian gradient
                    if constexpr (!BOUNDED) {
                        gmax = fmax(gmax, fabs(2.0 * g));
                    } else {   // projected gradient; epsilon-active holds of the first QP solve (oracle solve_one)
                        gmax = fmax(gmax, fabs(uk - proj(uk - 2.0 * g, lbv[c], ubv[c])));
                        sHold[k * NU + c] = (uk <= lbv[c] + beps && g > 0.0)   ? lbv[c]
                                            : (uk >= ubv[c] - beps && g < 0.0) ? ubv[c]
                                                                                : NAN;
                    }
                    nonfinite |= !isfinite(g);
                }
            }
        };
