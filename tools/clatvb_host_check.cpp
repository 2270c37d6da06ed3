// Stand-alone exercise of the host-only parts of the continuous latent-distance-network variational fit (csrc/nhp_clatvb.h):
// the argument checks that run before any launch, the ladder of step sizes and the sizing of the device state.  No HIP, no
// device.  Build and run under the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I networkhawkesprocesses.jl_amd/csrc \
//       tools/clatvb_host_check.cpp -o /tmp/clatvb_host_check && /tmp/clatvb_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "nhp_clatvb.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// Z of exactly the length the checks may read: an overrun is the sanitizer's to find
static std::vector<double> state(size_t N, size_t D)
{
    std::vector<double> Z(clatvb_z_doubles(N, D));
    for (size_t i = 0; i < Z.size(); ++i) Z[i] = 0.1 * (double)(i % 7) - 0.3;
    return Z;
}

static int args(int64_t N, const double *net, const double *lat, int32_t D, int32_t J, bool dense, const double *Z, char *msg, size_t cap)
{
    return clatvb_check_args("clatvb", N, net, lat, D, J, dense, Z, msg, cap);
}

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    char msg[256];
    const double net[2] = {0.3, 30.0}, lat[3] = {1.3, 0.2, 1.5};
    for (size_t N : {(size_t)1, (size_t)3, (size_t)70})
        for (size_t D : {(size_t)1, (size_t)2, (size_t)8}) {
            std::vector<double> Z = state(N, D);
            const int32_t d = (int32_t)D;
            EXPECT(args((int64_t)N, net, lat, d, 4, false, Z.data(), msg, sizeof msg) == CLATVB_OK && msg[0] == 0);
            EXPECT(args((int64_t)N, net, lat, d, 0, false, Z.data(), msg, sizeof msg) == CLATVB_OK);
            EXPECT(args((int64_t)N, net, lat, d, 64, false, Z.data(), msg, sizeof msg) == CLATVB_OK);
            EXPECT(args((int64_t)N, net, lat, d, 4, true, Z.data(), msg, sizeof msg) == CLATVB_EINVAL && std::strstr(msg, "DENSE"));
            EXPECT(args((int64_t)N, nullptr, lat, d, 4, false, Z.data(), msg, sizeof msg) == CLATVB_EINVAL);
            EXPECT(args((int64_t)N, net, nullptr, d, 4, false, Z.data(), msg, sizeof msg) == CLATVB_EINVAL);
            EXPECT(args((int64_t)N, net, lat, d, 4, false, nullptr, msg, sizeof msg) == CLATVB_EINVAL && std::strstr(msg, "NULL"));
            EXPECT(args((int64_t)N, net, lat, d, -1, false, Z.data(), msg, sizeof msg) == CLATVB_EINVAL && std::strstr(msg, "ascent_steps"));
            EXPECT(args((int64_t)N, net, lat, d, 65, false, Z.data(), msg, sizeof msg) == CLATVB_EINVAL && std::strstr(msg, "ascent_steps"));
            for (double v : {0.0, -2.0, nan, inf}) {
                for (int j = 0; j < 2; ++j) {
                    double bad[2] = {net[0], net[1]};
                    bad[j] = v;
                    EXPECT(args((int64_t)N, bad, lat, d, 4, false, Z.data(), msg, sizeof msg) == CLATVB_EINVAL && std::strstr(msg, "spike"));
                }
                for (int j : {0, 2}) {
                    double bad[3] = {lat[0], lat[1], lat[2]};
                    bad[j] = v;
                    EXPECT(args((int64_t)N, net, bad, d, 4, false, Z.data(), msg, sizeof msg) == CLATVB_EINVAL && std::strstr(msg, "sigma"));
                }
            }
            for (double v : {nan, inf, -inf}) {
                double bad[3] = {lat[0], v, lat[2]};
                EXPECT(args((int64_t)N, net, bad, d, 4, false, Z.data(), msg, sizeof msg) == CLATVB_EINVAL && std::strstr(msg, "mu_b"));
                for (size_t at : {(size_t)0, N * D - 1, N * D}) {                                          // first and last position, the offset
                    std::vector<double> z = Z;
                    z[at] = v;
                    EXPECT(args((int64_t)N, net, lat, d, 4, false, z.data(), msg, sizeof msg) == CLATVB_EINVAL && std::strstr(msg, "finite"));
                    EXPECT((std::strstr(msg, "b_v") != nullptr) == (at == N * D));
                }
            }
            double neg[3] = {lat[0], -3.0, lat[2]};                                                        // μb of either sign is fine
            EXPECT(args((int64_t)N, net, neg, d, 4, false, Z.data(), msg, sizeof msg) == CLATVB_OK);
        }
    // Z on the device: the same checks without reading Z (here a pointer to one double, which must not be read past)
    {
        const double one_z = nan;
        auto dev = [&](int64_t N, const double *n2, const double *l3, int32_t D, int32_t J, bool dense) {
            return clatvb_check_args("clatvb", N, n2, l3, D, J, dense, &one_z, msg, sizeof msg, true);
        };
        EXPECT(dev(70, net, lat, 3, 4, false) == CLATVB_OK && msg[0] == 0);
        EXPECT(dev(70, net, lat, 0, 4, false) == CLATVB_EINVAL && dev(70, net, lat, 9, 4, false) == CLATVB_EINVAL);
        EXPECT(dev(70, net, lat, 3, -1, false) == CLATVB_EINVAL && dev(70, net, lat, 3, 65, false) == CLATVB_EINVAL);
        EXPECT(dev(70, net, lat, 3, 4, true) == CLATVB_EINVAL);
        EXPECT(clatvb_check_args("clatvb", 70, net, lat, 3, 4, false, nullptr, msg, sizeof msg, true) == CLATVB_EINVAL);
    }
    // D outside 1..8 is refused before Z's length is formed (Z may then be anything, here a single double)
    const double one = 1.0;
    for (int32_t D : {0, -3, 9, 1 << 30}) EXPECT(args(3, net, lat, D, 4, false, &one, msg, sizeof msg) == CLATVB_EINVAL && std::strstr(msg, "n_dims"));
    // the ladder: τ = 1/(N + 1/σ²), every rung τ with another exponent, the current point last
    for (int64_t N : {(int64_t)1, (int64_t)12, (int64_t)1024})
        for (double s : {0.5, 1.0, 3.0}) {
            double t[CLATVB_SLOTS];
            clatvb_ladder(N, s, t);
            const double tau = 1.0 / ((double)N + 1.0 / (s * s));
            EXPECT(t[0] == 4.0 * tau && t[1] == tau && t[CLATVB_RUNGS] == 0.0);
            for (int r = 1; r < CLATVB_RUNGS; ++r) EXPECT(t[r] * 4.0 == t[r - 1] && t[r] > 0.0);
        }
    // the state: Q has three planes and no trailing pair
    for (size_t N : {(size_t)1, (size_t)3, (size_t)70}) {
        const size_t NN = N * N;
        std::vector<double> Q(3 * NN), k1(NN, 2.0), n1(NN, 1.5);
        for (size_t i = 0; i < NN; ++i) { Q[i] = 0.5; Q[NN + i] = 20.0; Q[2 * NN + i] = 0.25; }
        EXPECT(clatvb_check_state("clatvb", N, true, Q.data(), k1.data(), n1.data(), msg, sizeof msg) == CLATVB_OK && msg[0] == 0);
        EXPECT(clatvb_check_state("clatvb", N, true, nullptr, k1.data(), n1.data(), msg, sizeof msg) == CLATVB_EINVAL);
        std::vector<double> junk(3 * NN, -7.0);                     // without a state nothing of the planes is read
        EXPECT(clatvb_check_state("clatvb", N, false, junk.data(), nullptr, nullptr, msg, sizeof msg) == CLATVB_OK);
        EXPECT(clatvb_check_state("clatvb", N, true, junk.data(), k1.data(), n1.data(), msg, sizeof msg) == CLATVB_EINVAL);
        for (double v : {-1e-9, 1.0 + 1e-9, nan, inf}) {
            std::vector<double> q = Q;
            q.back() = v;
            EXPECT(clatvb_check_state("clatvb", N, true, q.data(), k1.data(), n1.data(), msg, sizeof msg) == CLATVB_EINVAL && std::strstr(msg, "rho_v"));
        }
        std::vector<double> ends = Q;
        ends[2 * NN] = 0.0; ends.back() = 1.0;                      // the closed ends are allowed
        EXPECT(clatvb_check_state("clatvb", N, true, ends.data(), k1.data(), n1.data(), msg, sizeof msg) == CLATVB_OK);
        char tiny[8];                                               // a short message buffer is cut, not overrun
        ends.back() = 2.0;
        EXPECT(clatvb_check_state("clatvb", N, true, ends.data(), k1.data(), n1.data(), tiny, sizeof tiny) == CLATVB_EINVAL && std::strlen(tiny) == sizeof tiny - 1);
        for (size_t D : {(size_t)1, (size_t)3, (size_t)8})
            for (size_t planes : {(size_t)2, (size_t)3}) {
                const size_t P = N + planes * NN, blocks = 1024, z = N * D + 1;
                const size_t st = 3 * P + 3 * NN + z + N + 8 * blocks, sc = NN + z + N + 9 * N + 11 + 64;
                EXPECT(clatvb_z_doubles(N, D) == z);
                EXPECT(clatvb_state_doubles(P, N, D, blocks) == st);
                EXPECT(clatvb_scratch_doubles(N, D) == sc);
                EXPECT(clatvb_reserve_doubles(P, N, D, blocks) == 2 * st + sc + 2 * CLATVB_OUT);
                EXPECT(clatvb_loglik_doubles(N, D) == 2 * NN + 3 * z + 2 * N + 11 + 1);
            }
    }
    EXPECT(CLATVB_OUT == 76 && CLATVB_STATS_FIXED == 19 && CLATVB_SLOTS == 9 && CLATVB_SC == 11);
    std::printf(failures ? "%d check(s) failed\n" : "clatvb host checks passed\n", failures);
    return failures ? 1 : 0;
}
