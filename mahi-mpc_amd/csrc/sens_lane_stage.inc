// sens_lane_stage.inc -- the text the sensitivity kernels share: the instance prologue and the backward stage of the
// one-lane-per-instance sweeps (gain_sweep.h, adjoint_sweep.h; the recursion is stated at the top of gain_sweep.h).
//
// This is kernel text, not a header: it is compiled into each kernel from here, the way sqp_group.h compiles
// sqp_group_body.inc into its three kernels, because a __device__ function holding the stage changes the register allocation, the scratch and
// in some instantiations the FP64 operation counts of every kernel that calls it (DESIGN.md 3j).  Set MMPC_SENS_PART
// and include the file inside the kernel; the file undefines the macro again.
//
// Every part expects the kernel's constants NX, NU, K, NQ, NA, NP (NP only in the stage parts), its template
// arguments Model, EXACT, BOUNDED, XB, and in scope:
//   p (GainParamsOf<XB> or AdjointParamsOf<XB>: the SensParams head, p.xb with XB), b (the instance), N, h,
//   v (the instance's V), w (its weights row), tr (its targets).
//
// MMPC_SENS_PART 0 -- the instance prologue (all three kernels).
//   defines: Q[NX], R[NU], Rm[NU], lb[NU], ub[NU] (the bounds +-INFINITY unless BOUNDED and given), up[NU] (u_prev),
//            fin (== 0.0 while x_N, u_prev and the weights are finite: the inputs no pivot ever sees).
//
// MMPC_SENS_PART 1 -- stage k of the backward sweep, from the model evaluation through the gains G_k.
//   expects: part 0's names, k, exact (this pass runs the exact Hessian), P[NP] = P_{k+1} (packed, gain_sym) and
//            lam[NX] = lam_k; XB adds beta(x_{k+1}) to lam and D(x_{k+1}) to P in place.
//   defines: x[NX], u[NU], J[NX][K] = [A_k | B_k], nuk[NX], M[NP] = M_yy, Muu[NU][NU] (its Cholesky factor) with
//            il[NU], Mus[NU][K], held[NU], G[NU][K], chk (stays == 0.0 while the stage is finite and, with XB, inside
//            its bounds);
//   updates: lam = lam_{k-1};  ok = the factorisation's pivots were > 0 and finite.
//
// MMPC_SENS_PART 2 -- P_k = M_ss + M_su G_k with its finite check.
//   expects: part 1's names;  updates: P = P_k, chk.  The kernel then sets ok = ok && chk == 0.0.
#if MMPC_SENS_PART == 0
    double Q[NX], R[NU], Rm[NU], lb[NU], ub[NU], up[NU];
    double fin = 0.0;
#pragma unroll
    for (int r = 0; r < NX; ++r) {
        Q[r] = w[r];
        fin += gain_nonfinite(v[(int64_t)N * K + r]) + gain_nonfinite(Q[r]);
    }
#pragma unroll
    for (int c = 0; c < NU; ++c) {
        R[c] = w[NX + c];
        Rm[c] = w[NX + NU + c];
        up[c] = p.u_prev[b * NU + c];
        fin += gain_nonfinite(up[c]) + gain_nonfinite(R[c]) + gain_nonfinite(Rm[c]);
        lb[c] = (BOUNDED && p.u_lb) ? p.u_lb[b * p.b_stride + c] : -INFINITY;
        ub[c] = (BOUNDED && p.u_ub) ? p.u_ub[b * p.b_stride + c] : INFINITY;
    }
#elif MMPC_SENS_PART == 1
            double x[NX], u[NU], xd[NX], fx[NX * NX], fu[NX * NU];
#pragma unroll
            for (int r = 0; r < NX; ++r) x[r] = v[k * K + r];
#pragma unroll
            for (int c = 0; c < NU; ++c) u[c] = v[k * K + NX + c];
            model_eval_jac<Model>(x, u, xd, fx, fu);
            double J[NX][K], nuk[NX], chk = 0.0;   // J = [A_k | B_k]
            [[maybe_unused]] double Du[NU];
            if constexpr (XB) {   // lam_k gets beta(x_{k+1}), P_{k+1} gets D(x_{k+1}) in place; D(u_k) for M_uu
                bool in = true;
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    double be, D;
                    in = xb_terms(v[(k + 1) * K + r], p.xb.x_lb[r], p.xb.x_ub[r], p.xb.mu, p.xb.cap, be, D) && in;
                    lam[r] += be;
                    P[gain_sym(r, r, K)] += D;
                }
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    double be;
                    Du[c] = 0.0;
                    if (k >= p.n_pin) in = xb_terms(u[c], lb[c], ub[c], p.xb.mu, p.xb.cap, be, Du[c]) && in;
                }
                chk += in ? 0.0 : NAN;
            }
#pragma unroll
            for (int r = 0; r < NX; ++r) {
#pragma unroll
                for (int c = 0; c < NX; ++c) J[r][c] = (r == c ? 1.0 : 0.0) + h * fx[r * NX + c];
#pragma unroll
                for (int c = 0; c < NU; ++c) J[r][NX + c] = h * fu[r * NU + c];
                const double e = x[r] + h * xd[r] - tr[k * NX + r];
                nuk[r] = 2.0 * Q[r] * e + lam[r];
                chk += gain_nonfinite(nuk[r]);   // a non-finite target fails the instance under either Hessian
            }
#pragma unroll
            for (int c = 0; c < NX; ++c) {   // lam_{k-1} = A_k^T nu_k
                double s = 0.0;
#pragma unroll
                for (int r = 0; r < NX; ++r) s += J[r][c] * nuk[r];
                lam[c] = s;
            }
            // M_yy = C^T P C + S_k, column by column of P C
            double M[NP];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                double t[K];
#pragma unroll
                for (int a = 0; a < K; ++a) {
                    double s = j >= NX ? P[gain_sym(a, j, K)] : 0.0;
#pragma unroll
                    for (int q = 0; q < NX; ++q) s += P[gain_sym(a, q, K)] * J[q][j];
                    t[a] = s;
                }
#pragma unroll
                for (int i = 0; i <= j; ++i) {
                    double s = i >= NX ? t[i] : 0.0;
#pragma unroll
                    for (int a = 0; a < NX; ++a) s += J[a][i] * t[a];
#pragma unroll
                    for (int r = 0; r < NX; ++r) s += 2.0 * Q[r] * J[r][i] * J[r][j];
                    M[gain_sym(i, j, K)] = s;
                }
            }
            if constexpr (EXACT) {
                if (exact) {
                    double la[NA], W[K * K];
#pragma unroll
                    for (int s2 = 0; s2 < NA; ++s2) la[s2] = h * nuk[NQ + s2];
                    Model::eval_hess(x, u, la, W);
#pragma unroll
                    for (int i = 0; i < K; ++i)
#pragma unroll
                        for (int j = i; j < K; ++j) M[gain_sym(i, j, K)] += W[i * K + j];
                }
            }
            double Muu[NU][NU], Mus[NU][K], il[NU];
            bool held[NU];
#pragma unroll
            for (int c = 0; c < NU; ++c) held[c] = gain_held<BOUNDED && !XB>(k, p.n_pin, u[c], lb[c], ub[c]);
#pragma unroll
            for (int c = 0; c < NU; ++c) {
#pragma unroll
                for (int d = 0; d < NU; ++d) {
                    double m = M[gain_sym(NX + c, NX + d, K)] + (c == d ? 2.0 * R[c] + 2.0 * Rm[c] : 0.0);
                    if constexpr (XB) m += c == d ? Du[c] : 0.0;
                    Muu[c][d] = (held[c] || held[d]) ? (c == d ? 1.0 : 0.0) : m;
                }
#pragma unroll
                for (int j = 0; j < NX; ++j) Mus[c][j] = held[c] ? 0.0 : M[gain_sym(j, NX + c, K)];
#pragma unroll
                for (int d = 0; d < NU; ++d) Mus[c][NX + d] = (c == d && !held[c]) ? -2.0 * R[c] : 0.0;
            }
            ok = gain_chol<NU>(Muu, il);
            double G[NU][K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                double m[NU], g[NU];
#pragma unroll
                for (int c = 0; c < NU; ++c) m[c] = Mus[c][j];
                gain_solve<NU>(Muu, il, m, g);
#pragma unroll
                for (int c = 0; c < NU; ++c) G[c][j] = held[c] ? 0.0 : g[c];
            }
#elif MMPC_SENS_PART == 2
            // P_k = M_ss + M_su G_k
#pragma unroll
            for (int i = 0; i < K; ++i)
#pragma unroll
                for (int j = i; j < K; ++j) {
                    double s = (j < NX) ? M[gain_sym(i, j, K)] : ((i == j) ? 2.0 * R[i - (i >= NX ? NX : 0)] : 0.0);
#pragma unroll
                    for (int c = 0; c < NU; ++c) s += Mus[c][i] * G[c][j];
                    P[gain_sym(i, j, K)] = s;
                    chk += gain_nonfinite(s);
                }
#else
#error "sens_lane_stage.inc: set MMPC_SENS_PART to 0 (prologue), 1 (stage through G_k) or 2 (P_k) before the include"
#endif
#undef MMPC_SENS_PART
