// Stand-alone exercise of the host-only parts of the continuous block-network variational fit (csrc/nhp_csbmvb.h): the
// argument checks that run before any launch and the sizing of the device state.  No HIP, no device.  Build and run under
// the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I networkhawkesprocesses.jl_amd/csrc \
//       tools/csbmvb_host_check.cpp -o /tmp/csbmvb_host_check && /tmp/csbmvb_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "nhp_csbmvb.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// B of exactly the length the checks may read: an overrun is the sanitizer's to find
static std::vector<double> block_state(size_t N, size_t K)
{
    std::vector<double> B(csbmvb_b_doubles(N, K), 2.0);
    for (size_t i = 0; i < N * K; ++i) B[2 * K * K + K + i] = 1.0 / (double)K;
    return B;
}

static int args(int64_t N, int32_t K, const double *net, const double *sbm, int32_t every, int64_t step0, bool dense, const double *B, char *msg,
                size_t cap)
{
    return csbmvb_check_args("csbmvb", N, net, sbm, K, every, step0, dense, B, msg, cap);
}

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    char msg[256];
    const double net[2] = {0.3, 30.0}, sbm[3] = {1.5, 2.5, 1.2};
    for (size_t N : {(size_t)1, (size_t)3, (size_t)70})
        for (size_t K : {(size_t)1, (size_t)2, (size_t)5, (size_t)64}) {
            std::vector<double> B = block_state(N, K);
            const int32_t k = (int32_t)K;
            EXPECT(args((int64_t)N, k, net, sbm, 1, 0, false, B.data(), msg, sizeof msg) == CSBMVB_OK && msg[0] == 0);
            EXPECT(args((int64_t)N, k, net, sbm, 7, 12, false, B.data(), msg, sizeof msg) == CSBMVB_OK);
            EXPECT(args((int64_t)N, k, net, sbm, 1, 0, true, B.data(), msg, sizeof msg) == CSBMVB_EINVAL && std::strstr(msg, "DENSE"));
            EXPECT(args((int64_t)N, k, nullptr, sbm, 1, 0, false, B.data(), msg, sizeof msg) == CSBMVB_EINVAL);
            EXPECT(args((int64_t)N, k, net, nullptr, 1, 0, false, B.data(), msg, sizeof msg) == CSBMVB_EINVAL);
            EXPECT(args((int64_t)N, k, net, sbm, 1, 0, false, nullptr, msg, sizeof msg) == CSBMVB_EINVAL && std::strstr(msg, "NULL"));
            EXPECT(args((int64_t)N, k, net, sbm, 0, 0, false, B.data(), msg, sizeof msg) == CSBMVB_EINVAL && std::strstr(msg, "labels_every"));
            EXPECT(args((int64_t)N, k, net, sbm, 1, -1, false, B.data(), msg, sizeof msg) == CSBMVB_EINVAL && std::strstr(msg, "step0"));
            EXPECT(args(0, k, net, sbm, 1, 0, false, B.data(), msg, sizeof msg) == CSBMVB_EINVAL);
            for (double v : {0.0, -2.0, nan, inf}) {
                for (int j = 0; j < 2; ++j) {
                    double bad[2] = {net[0], net[1]};
                    bad[j] = v;
                    EXPECT(args((int64_t)N, k, bad, sbm, 1, 0, false, B.data(), msg, sizeof msg) == CSBMVB_EINVAL && std::strstr(msg, "spike"));
                }
                for (int j = 0; j < 3; ++j) {
                    double bad[3] = {sbm[0], sbm[1], sbm[2]};
                    bad[j] = v;
                    EXPECT(args((int64_t)N, k, net, bad, 1, 0, false, B.data(), msg, sizeof msg) == CSBMVB_EINVAL && std::strstr(msg, "priors"));
                }
                for (size_t at : {(size_t)0, K * K - 1, K * K, 2 * K * K - 1, 2 * K * K, 2 * K * K + K - 1}) {      // αv, βv, γv: first and last
                    std::vector<double> b = B;
                    b[at] = v;
                    EXPECT(args((int64_t)N, k, net, sbm, 1, 0, false, b.data(), msg, sizeof msg) == CSBMVB_EINVAL);
                }
            }
            for (double v : {-1e-9, nan, 1.0 / (double)K + 1e-9}) {                                        // a row of m off the simplex
                std::vector<double> b = B;
                b.back() = v;
                EXPECT(args((int64_t)N, k, net, sbm, 1, 0, false, b.data(), msg, sizeof msg) == CSBMVB_EINVAL && std::strstr(msg, "m"));
            }
        }
    // B on the device: the same checks without reading B (here a pointer to one double, which must not be read past)
    {
        const double one_b = 1.0;
        auto dev = [&](int64_t N, int32_t K, const double *n2, const double *s3, int32_t every, int64_t step0, bool dense) {
            return csbmvb_check_args("csbmvb", N, n2, s3, K, every, step0, dense, &one_b, msg, sizeof msg, true);
        };
        EXPECT(dev(70, 5, net, sbm, 1, 0, false) == CSBMVB_OK && msg[0] == 0);
        EXPECT(dev(70, 5, net, sbm, 0, 0, false) == CSBMVB_EINVAL && std::strstr(msg, "labels_every"));
        EXPECT(dev(70, 5, net, sbm, 1, -1, false) == CSBMVB_EINVAL && dev(70, 5, net, sbm, 1, 0, true) == CSBMVB_EINVAL);
        EXPECT(dev(70, 0, net, sbm, 1, 0, false) == CSBMVB_EINVAL && dev(70, 65, net, sbm, 1, 0, false) == CSBMVB_EINVAL);
        EXPECT(dev(0, 5, net, sbm, 1, 0, false) == CSBMVB_EINVAL);
        EXPECT(dev(400, 64, net, sbm, 1, 0, false) == CSBMVB_ENOTIMPL && std::strstr(msg, "LDS"));
        EXPECT(csbmvb_check_args("csbmvb", 70, net, sbm, 5, 1, 0, false, nullptr, msg, sizeof msg, true) == CSBMVB_EINVAL);
        for (double v : {0.0, -2.0, nan, inf})
            for (int j = 0; j < 3; ++j) {
                double bad[3] = {sbm[0], sbm[1], sbm[2]};
                bad[j] = v;
                EXPECT(dev(70, 5, net, bad, 1, 0, false) == CSBMVB_EINVAL && std::strstr(msg, "priors"));
            }
    }
    // K outside 1..64 is refused before B's offsets are formed (B may then be anything, here a single double)
    const double one = 1.0;
    for (int32_t K : {0, -3, 65, 1 << 30}) EXPECT(args(3, K, net, sbm, 1, 0, false, &one, msg, sizeof msg) == CSBMVB_EINVAL && std::strstr(msg, "n_blocks"));
    // a sweep that does not fit in LDS: not implemented, and the message names the need
    {
        const size_t N = 400, K = 64;
        std::vector<double> B = block_state(N, K);
        EXPECT(sbmvb_sweep_lds_bytes(N, K) > (size_t)SBMVB_LDS_LIMIT);
        EXPECT(args((int64_t)N, (int32_t)K, net, sbm, 1, 0, false, B.data(), msg, sizeof msg) == CSBMVB_ENOTIMPL && std::strstr(msg, "LDS"));
    }
    // the state: Q has three planes and no trailing pair
    for (size_t N : {(size_t)1, (size_t)3, (size_t)70}) {
        const size_t NN = N * N;
        std::vector<double> Q(3 * NN), k1(NN, 2.0), n1(NN, 1.5);
        for (size_t i = 0; i < NN; ++i) { Q[i] = 0.5; Q[NN + i] = 20.0; Q[2 * NN + i] = 0.25; }
        EXPECT(csbmvb_check_state("csbmvb", N, true, Q.data(), k1.data(), n1.data(), msg, sizeof msg) == CSBMVB_OK && msg[0] == 0);
        EXPECT(csbmvb_check_state("csbmvb", N, true, nullptr, k1.data(), n1.data(), msg, sizeof msg) == CSBMVB_EINVAL);
        std::vector<double> junk(3 * NN, -7.0);                     // without a state nothing of the planes is read
        EXPECT(csbmvb_check_state("csbmvb", N, false, junk.data(), nullptr, nullptr, msg, sizeof msg) == CSBMVB_OK);
        EXPECT(csbmvb_check_state("csbmvb", N, true, junk.data(), k1.data(), n1.data(), msg, sizeof msg) == CSBMVB_EINVAL);
        for (double v : {-1e-9, 1.0 + 1e-9, nan, inf}) {
            std::vector<double> q = Q;
            q.back() = v;
            EXPECT(csbmvb_check_state("csbmvb", N, true, q.data(), k1.data(), n1.data(), msg, sizeof msg) == CSBMVB_EINVAL && std::strstr(msg, "rho_v"));
        }
        std::vector<double> ends = Q;
        ends[2 * NN] = 0.0; ends.back() = 1.0;                      // the closed ends are allowed
        EXPECT(csbmvb_check_state("csbmvb", N, true, ends.data(), k1.data(), n1.data(), msg, sizeof msg) == CSBMVB_OK);
        char tiny[8];                                               // a short message buffer is cut, not overrun
        ends.back() = 2.0;
        EXPECT(csbmvb_check_state("csbmvb", N, true, ends.data(), k1.data(), n1.data(), tiny, sizeof tiny) == CSBMVB_EINVAL && std::strlen(tiny) == sizeof tiny - 1);
        for (size_t K : {(size_t)1, (size_t)5, (size_t)64})
            for (size_t planes : {(size_t)2, (size_t)3}) {
                const size_t P = N + planes * NN, blocks = 1024, b = 2 * K * K + K + N * K, t = 2 * K * K + K;
                EXPECT(csbmvb_b_doubles(N, K) == b && csbmvb_t_doubles(K) == t);
                EXPECT(csbmvb_state_doubles(P, N, K, blocks) == 3 * P + 3 * NN + b + t + 8 * blocks);
                EXPECT(csbmvb_scratch_doubles(N, K) == 5 * K * K + K + 3 * N * K);
                EXPECT(csbmvb_reserve_doubles(P, N, K, blocks) == 2 * (3 * P + 3 * NN + b + t + 8 * blocks) + 5 * K * K + K + 3 * N * K + 2 * CSBMVB_OUT);
            }
    }
    EXPECT(CSBMVB_OUT == 13 && CSBMVB_STATS == 21);
    EXPECT(csbmvb_dir_const(1.0, 1) == 0.0 && std::fabs(csbmvb_dir_const(1.0, 3) - std::log(2.0)) < 1e-15);
    std::printf(failures ? "%d check(s) failed\n" : "csbmvb host checks passed\n", failures);
    return failures ? 1 : 0;
}
