// Microbenchmark (diagnostic, not product): the feedback kernel of csrc/rti_sweep.h at several ring depths D -- the
// number of stage records a lane keeps in registers, i.e. how many stages ahead of its use a record's load is issued
// (D - 1).  Records, plan and measured states are synthetic and small (|G|, |A - I| ~ 1e-2), so every step stays finite;
// the time does not depend on the data.  Per (shape, B, D): 20 back-to-back launches, median of 7 blocks, in us.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -mllvm -pragma-unroll-threshold=1000000 -mllvm -sgpr-regalloc=basic \
//         -I mahi-mpc_amd/csrc -o tools/ubench/rti_ring tools/ubench/rti_ring.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "rti_sweep.h"

using namespace mmpc;

#define CK(x)                                                                  \
    do {                                                                       \
        hipError_t e_ = (x);                                                   \
        if (e_ != hipSuccess) {                                                \
            std::printf("%s: %s\n", #x, hipGetErrorString(e_));                \
            return 1;                                                          \
        }                                                                      \
    } while (0)

template <int NX, int NU, int D>
int run(const char* name, int N, int64_t B) {
    constexpr int K = NX + NU, RD = rti_rec_doubles(NX, NU);
    const int64_t blocks = (B + 63) / 64, NV = (int64_t)NX * (N + 1) + (int64_t)NU * N;
    const size_t nrec = blocks * rti_rec_block_doubles(NX, NU, N), nundo = blocks * rti_undo_block_doubles(NX, NU, N);
    std::vector<double> rec(nrec), V(B * NV), x0(B * NX);
    uint64_t sd = 88172645463325252ull;
    auto rnd = [&] { sd ^= sd << 13; sd ^= sd >> 7; sd ^= sd << 17; return (double)(sd >> 11) / 9007199254740992.0 - 0.5; };
    for (int64_t g = 0; g < blocks; ++g)
        for (int k = 0; k < N; ++k)
            for (int i = 0; i < RD; ++i)
                for (int l = 0; l < 64; ++l) {
                    const int row = i / (K + 1), col = i % (K + 1);
                    const double id = (row >= NU && col == row - NU) ? 1.0 : 0.0;   // A_k = I + small
                    rec[((g * N + k) * RD + i) * 64 + l] = id + 2e-2 * rnd();
                }
    for (auto& v : V) v = rnd();
    for (int64_t b = 0; b < B; ++b)
        for (int r = 0; r < NX; ++r) x0[b * NX + r] = V[b * NV + r] + 1e-2 * rnd();
    double *drec, *dundo, *dV, *dV0, *dx0, *du0, *dsi;
    int32_t *dws, *dst;
    CK(hipMalloc(&drec, nrec * 8));
    CK(hipMalloc(&dundo, nundo * 8));
    CK(hipMalloc(&dV, V.size() * 8));
    CK(hipMalloc(&dV0, V.size() * 8));
    CK(hipMalloc(&dx0, x0.size() * 8));
    CK(hipMalloc(&du0, B * NU * 8));
    CK(hipMalloc(&dsi, B * 8));
    CK(hipMalloc(&dws, blocks * 64 * 4));
    CK(hipMalloc(&dst, B * 4));
    CK(hipMemcpy(drec, rec.data(), nrec * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dV0, V.data(), V.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dx0, x0.data(), x0.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemset(dws, 0, blocks * 64 * 4));
    RtiFeedbackParams p{};
    p.B = B, p.N = N, p.x0 = dx0, p.V = dV, p.u0 = du0, p.step_inf = dsi, p.status = dst;
    p.rec = drec, p.undo = dundo, p.ws_status = dws;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::vector<float> t;
    for (int blk = 0; blk < 8; ++blk) {   // the first block is the warm-up
        CK(hipMemcpy(dV, dV0, V.size() * 8, hipMemcpyDeviceToDevice));
        CK(hipEventRecord(e0, nullptr));
        for (int i = 0; i < 20; ++i)
            rti_feedback_lane_kernel<NX, NU, false, D><<<dim3((unsigned)blocks), 64, 0, nullptr>>>(p);
        CK(hipEventRecord(e1, nullptr));
        CK(hipEventSynchronize(e1));
        CK(hipGetLastError());
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (blk) t.push_back(ms / 20 * 1000);
    }
    std::vector<int32_t> st(B);
    CK(hipMemcpy(st.data(), dst, B * 4, hipMemcpyDeviceToHost));
    int64_t bad = 0;
    for (auto s : st) bad += s != 0;
    std::sort(t.begin(), t.end());
    std::printf("{\"shape\": \"%s\", \"N\": %d, \"B\": %lld, \"D\": %d, \"us\": %.2f, \"max_minus_min\": %.2f, \"failed\": %lld}\n",
                name, N, (long long)B, D, t[t.size() / 2], t.back() - t.front(), (long long)bad);
    for (void* q : {(void*)drec, (void*)dundo, (void*)dV, (void*)dV0, (void*)dx0, (void*)du0, (void*)dsi, (void*)dws,
                    (void*)dst})
        CK(hipFree(q));
    return 0;
}

int main() {
    for (int64_t B : {64, 4096}) {
        if (run<4, 2, 1>("cfg2", 30, B) || run<4, 2, 2>("cfg2", 30, B) || run<4, 2, 3>("cfg2", 30, B) ||
            run<4, 2, 4>("cfg2", 30, B))
            return 1;
    }
    if (run<8, 4, 1>("cfg3", 50, 4096) || run<8, 4, 2>("cfg3", 50, 4096)) return 1;
    return 0;
}
