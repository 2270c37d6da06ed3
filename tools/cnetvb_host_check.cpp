// Stand-alone exercise of the host-only parts of the continuous network variational fit (csrc/nhp_cnetvb.h): the argument
// checks that run before any launch and the sizing of the device state.  No HIP, no device.  Build and run under the host
// sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I networkhawkesprocesses.jl_amd/csrc \
//       tools/cnetvb_host_check.cpp -o /tmp/cnetvb_host_check && /tmp/cnetvb_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "nhp_cnetvb.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

struct state {
    std::vector<double> Q, k1, n1;       // exactly the lengths the checks may read: an overrun is the sanitizer's to find
    explicit state(size_t N) : Q(3 * N * N + 2), k1(N * N, 2.0), n1(N * N, 1.5)
    {
        const size_t NN = N * N;
        for (size_t i = 0; i < NN; ++i) { Q[i] = 0.5; Q[NN + i] = 20.0; Q[2 * NN + i] = 0.25; }
        Q[3 * NN] = 2.0; Q[3 * NN + 1] = 3.0;
    }
};

static int run(size_t N, bool dense, bool st, state &s, char *msg, size_t cap)
{
    return cnetvb_check_state("cnetvb", N, dense, st, s.Q.data(), s.k1.data(), s.n1.data(), msg, cap);
}

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    char msg[256];
    const double ok[4] = {0.3, 30.0, 1.5, 2.5};
    EXPECT(cnetvb_check_net("cnetvb", ok, false, msg, sizeof msg) == CNETVB_OK && msg[0] == 0);
    EXPECT(cnetvb_check_net("cnetvb", nullptr, false, msg, sizeof msg) == CNETVB_EINVAL && std::strstr(msg, "NULL"));
    for (int j = 0; j < 4; ++j)
        for (double v : {0.0, -2.0, nan, inf}) {
            double bad[4] = {ok[0], ok[1], ok[2], ok[3]};
            bad[j] = v;
            EXPECT(cnetvb_check_net("cnetvb", bad, false, msg, sizeof msg) == CNETVB_EINVAL && std::strstr(msg, j < 2 ? "spike" : "network"));
            EXPECT(cnetvb_check_net("cnetvb", bad, true, msg, sizeof msg) == (j < 2 ? CNETVB_EINVAL : CNETVB_OK));      // dense: α, β ignored
        }
    for (size_t N : {(size_t)1, (size_t)3, (size_t)70}) {
        const size_t NN = N * N;
        state s(N);
        EXPECT(run(N, false, true, s, msg, sizeof msg) == CNETVB_OK && msg[0] == 0);
        EXPECT(run(N, false, false, s, msg, sizeof msg) == CNETVB_OK);
        EXPECT(cnetvb_check_state("cnetvb", N, false, false, nullptr, nullptr, nullptr, msg, sizeof msg) == CNETVB_EINVAL);
        // without a state only (αv, βv) are read: the planes may hold anything and the slab's tables may be missing
        state junk(N);
        for (size_t i = 0; i < 3 * NN; ++i) junk.Q[i] = -7.0;
        EXPECT(cnetvb_check_state("cnetvb", N, false, false, junk.Q.data(), nullptr, nullptr, msg, sizeof msg) == CNETVB_OK);
        EXPECT(run(N, false, true, junk, msg, sizeof msg) == CNETVB_EINVAL && std::strstr(msg, "kappa_v"));
        for (double v : {0.0, -1.0, nan, inf}) {
            for (size_t at : {3 * NN, 3 * NN + 1}) {
                state b(N);
                b.Q[at] = v;
                EXPECT(run(N, false, false, b, msg, sizeof msg) == CNETVB_EINVAL && std::strstr(msg, "alpha_v"));
                EXPECT(run(N, true, true, b, msg, sizeof msg) == CNETVB_OK);                  // a dense network passes them through
            }
            for (size_t plane : {(size_t)0, (size_t)1}) {
                state b(N);
                b.Q[plane * NN + NN - 1] = v;
                EXPECT(run(N, false, true, b, msg, sizeof msg) == CNETVB_EINVAL && std::strstr(msg, "kappa_v / nu_v"));
                EXPECT(run(N, true, true, b, msg, sizeof msg) == CNETVB_EINVAL);
            }
            state b(N);
            b.k1.back() = v;
            EXPECT(run(N, false, true, b, msg, sizeof msg) == CNETVB_EINVAL);
            b.k1.back() = 2.0; b.n1.front() = v;
            EXPECT(run(N, false, true, b, msg, sizeof msg) == CNETVB_EINVAL);
        }
        for (double v : {-1e-9, 1.0 + 1e-9, nan, inf}) {
            state b(N);
            b.Q[2 * NN] = v;
            EXPECT(run(N, false, true, b, msg, sizeof msg) == CNETVB_EINVAL && std::strstr(msg, "rho_v"));
            EXPECT(run(N, true, true, b, msg, sizeof msg) == CNETVB_OK);                      // a dense network ignores rho_v
        }
        state ends(N);
        ends.Q[2 * NN] = 0.0; ends.Q[3 * NN - 1] = 1.0;                                       // the closed ends are allowed
        EXPECT(run(N, false, true, ends, msg, sizeof msg) == CNETVB_OK);
        char tiny[8];                                                                         // a short message buffer is cut, not overrun
        ends.Q[2 * NN] = 2.0;
        EXPECT(run(N, false, true, ends, tiny, sizeof tiny) == CNETVB_EINVAL && std::strlen(tiny) == sizeof tiny - 1);
        // the sizing: two states of surrogate, S, R, Q (+ the logit's network term) and partial sums, and two sets of scalars
        for (size_t planes : {(size_t)2, (size_t)3}) {
            const size_t P = N + planes * NN, blocks = 1024;
            EXPECT(cnetvb_q_doubles(N) == 3 * NN + 3);
            EXPECT(cnetvb_state_doubles(P, N, blocks) == 3 * P + 3 * NN + 3 + 8 * blocks);
            EXPECT(cnetvb_reserve_doubles(P, N, blocks) == 2 * (3 * P + 3 * NN + 3 + 8 * blocks) + 16);
            // the standard fit's: surrogate, S, R and five partial sums per state, six scalars per evaluation
            EXPECT(cvb_state_doubles(P, blocks) == 3 * P + 5 * blocks);
            EXPECT(cvb_reserve_doubles(P, blocks) == 2 * (3 * P + 5 * blocks) + 12);
            // the bump allocator, carving as the drivers do: inside the block, in order, and `used` is what was handed out
            std::vector<double> block(cnetvb_reserve_doubles(P, N, blocks), 0.0);
            vb_bump mem(block.data());
            for (int s = 0; s < 2; ++s) {
                double *x = mem.take(P), *S = mem.take(P), *R = mem.take(P), *Q = mem.take(cnetvb_q_doubles(N)), *part = mem.take(8 * blocks);
                EXPECT(S == x + P && R == S + P && Q == R + P && part == Q + 3 * NN + 3);
                x[0] = part[8 * blocks - 1] = 1.0;                                            // both ends lie inside the block
            }
            double *out = mem.take(2 * CNETVB_OUT);
            out[2 * CNETVB_OUT - 1] = 1.0;
            EXPECT(mem.used() == block.size() && out + 2 * CNETVB_OUT == block.data() + block.size());
        }
    }
    const double pl = cnetvb_prior_logit(0.5, 20.0, 2.0, 1.5);
    EXPECT(std::fabs(pl - ((2.0 * std::log(1.5) - std::lgamma(2.0)) - (0.5 * std::log(20.0) - std::lgamma(0.5)))) < 1e-15);
    EXPECT(cnetvb_prior_logit(0.7, 3.0, 0.7, 3.0) == 0.0);
    EXPECT(std::fabs(cnetvb_beta_const(1.0, 1.0)) < 1e-15 && std::fabs(cnetvb_beta_const(2.0, 3.0) - std::log(12.0)) < 1e-14);
    std::printf(failures ? "%d check(s) failed\n" : "cnetvb host checks passed\n", failures);
    return failures ? 1 : 0;
}
