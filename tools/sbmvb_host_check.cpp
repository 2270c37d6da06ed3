// Stand-alone exercise of the host-only parts of the block-model VB / SVI entry points (csrc/nhp_sbmvb.h): the argument
// checks that run before any launch, the LDS need of the label sweep and the scratch sizing.  No HIP, no device.  Build and
// run under the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I networkhawkesprocesses.jl_amd/csrc \
//       tools/sbmvb_host_check.cpp -o /tmp/sbmvb_host_check && /tmp/sbmvb_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "nhp_sbmvb.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

struct state {
    std::vector<double> m, av, bv, gv;
    state(size_t N, size_t K) : m(N * K, 1.0 / (double)K), av(K * K, 1.5), bv(K * K, 2.5), gv(K, 1.2) {}
};

static int run(int64_t N, int32_t K, state &s, char *msg, size_t cap, double a = 1.0, double b = 1.0, double g = 1.0, int32_t every = 1)
{
    return sbmvb_check_args("sbmvb", N, K, a, b, g, every, s.m.data(), s.av.data(), s.bv.data(), s.gv.data(), msg, cap);
}

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    char msg[256];
    for (int64_t N : {1, 5, 130}) {
        for (int32_t K : {1, 3, 64}) {
            state s((size_t)N, (size_t)K);
            EXPECT(run(N, K, s, msg, sizeof msg) == NETVB_OK && msg[0] == 0);
            // one-hot rows with exact zeros are on the simplex
            for (size_t n = 0; n < (size_t)N; ++n)
                for (size_t k = 0; k < (size_t)K; ++k) s.m[n + k * (size_t)N] = k == n % (size_t)K ? 1.0 : 0.0;
            EXPECT(run(N, K, s, msg, sizeof msg) == NETVB_OK);
            const double keep = s.m[0];
            s.m[0] = keep + 1e-9;
            EXPECT(run(N, K, s, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "sums to"));
            s.m[0] = keep + 1e-14;                              // inside the 1e-12 the check allows
            EXPECT(run(N, K, s, msg, sizeof msg) == NETVB_OK);
            s.m[0] = nan;
            EXPECT(run(N, K, s, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "m["));
            s.m[0] = -1e-300;
            EXPECT(run(N, K, s, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "negative"));
            s.m[0] = keep;
            for (double v : {0.0, -1.0, nan, inf}) {
                s.av.back() = v;
                EXPECT(run(N, K, s, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "alpha_v"));
                s.av.back() = 1.5;
                s.bv.front() = v;
                EXPECT(run(N, K, s, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "beta_v"));
                s.bv.front() = 2.5;
                s.gv.back() = v;
                EXPECT(run(N, K, s, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "gamma_v_net"));
                s.gv.back() = 1.2;
                EXPECT(run(N, K, s, msg, sizeof msg, v) == NETVB_EINVAL && std::strstr(msg, "priors"));
                EXPECT(run(N, K, s, msg, sizeof msg, 1.0, v) == NETVB_EINVAL);
                EXPECT(run(N, K, s, msg, sizeof msg, 1.0, 1.0, v) == NETVB_EINVAL);
            }
            EXPECT(run(N, K, s, msg, sizeof msg, 1.0, 1.0, 1.0, 0) == NETVB_EINVAL && std::strstr(msg, "labels_every"));
            EXPECT(sbmvb_check_args("sbmvb", N, K, 1.0, 1.0, 1.0, 1, nullptr, s.av.data(), s.bv.data(), s.gv.data(), msg, sizeof msg) == NETVB_EINVAL);
            char tiny[8];                                       // a short message buffer is cut, not overrun
            s.m[0] = 7.0;
            EXPECT(run(N, K, s, tiny, sizeof tiny) == NETVB_EINVAL && std::strlen(tiny) == sizeof tiny - 1);
            // the sizing: the state twice (hats), five K x K tables and Eπ, m·D, U1, U0, and ρ̂v for SVI
            const size_t n = (size_t)N, k = (size_t)K, st = n * k + 2 * k * k + k;
            EXPECT(sbmvb_state_doubles(n, k) == st);
            EXPECT(sbmvb_param_doubles(n, k, false) == 2 * st + 5 * k * k + k + 3 * n * k);
            EXPECT(sbmvb_param_doubles(n, k, true) == sbmvb_param_doubles(n, k, false) + n * n);
        }
    }
    {
        state s(4, 1);
        EXPECT(run(4, 0, s, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "n_blocks"));
        EXPECT(run(4, 65, s, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "n_blocks"));
        EXPECT(run(0, 1, s, msg, sizeof msg) == NETVB_EINVAL);
    }
    EXPECT(sbmvb_pow2(1) == 1 && sbmvb_pow2(2) == 2 && sbmvb_pow2(3) == 4 && sbmvb_pow2(5) == 8 && sbmvb_pow2(33) == 64 && sbmvb_pow2(64) == 64);
    EXPECT(sbmvb_sweep_lds_bytes(1024, 8) == 8 * (1024 * 8 + 2048 + 20 * 8));
    EXPECT(sbmvb_sweep_lds_bytes(70, 64) == 8 * (70 * 64 + 140 + 20 * 64));
    EXPECT(sbmvb_sweep_table_bytes(8) == 2048 && sbmvb_sweep_table_bytes(64) == 131072);
    EXPECT(sbmvb_sweep_lds_bytes(70, 64) + sbmvb_sweep_table_bytes(64) > (size_t)SBMVB_LDS_LIMIT);   // K = 64: the tables stay global
    {                                                           // the LDS limit: refused with the byte count in the message
        const int64_t N = 400;
        const int32_t K = 64;
        state s((size_t)N, (size_t)K);
        char want[32];
        std::snprintf(want, sizeof want, "%zu bytes", sbmvb_sweep_lds_bytes((size_t)N, (size_t)K));
        EXPECT(sbmvb_sweep_lds_bytes((size_t)N, (size_t)K) == 221440);
        EXPECT(run(N, K, s, msg, sizeof msg) == NETVB_ENOTIMPL && std::strstr(msg, want));
        state fits(1024, 16);                                   // 8 (16384 + 2048 + 320) = 150016 <= 163840
        EXPECT(run(1024, 16, fits, msg, sizeof msg) == NETVB_OK);
        state over(1024, 18);
        EXPECT(run(1024, 18, over, msg, sizeof msg) == NETVB_ENOTIMPL);
    }
    std::printf(failures ? "%d check(s) failed\n" : "sbmvb host checks passed\n", failures);
    return failures ? 1 : 0;
}
