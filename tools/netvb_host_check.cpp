// Stand-alone exercise of the host-only parts of the network VB / SVI entry points (csrc/nhp_netvb.h): the argument checks
// that run before any launch, the SVI schedule's checks and the sizing of what the discrete variational fits reserve.
// No HIP, no device.  Build and run under the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I networkhawkesprocesses.jl_amd/csrc \
//       tools/netvb_host_check.cpp -o /tmp/netvb_host_check && /tmp/netvb_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "nhp_netvb.h"
#include "nhp_sbmvb.h"
#include "nhp_vb_bump.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

struct params {
    std::vector<double> av, bv, k0, n0, k1, n1, gv, rho;
    double na = 1.5, nb = 2.5;
    params(size_t N, size_t B) : av(N, 1.0), bv(N, 2.0), k0(N * N, 0.5), n0(N * N, 20.0), k1(N * N, 2.0), n1(N * N, 1.5),
                                 gv(N * N * B, 1.0), rho(N * N, 0.25) {}
};

static int run(const netvb_priors &q, double dt, int64_t N, int64_t B, int32_t steps, params &p, char *msg, size_t cap, bool net_null = false)
{
    return netvb_check_args("netvb", q, dt, N, B, steps, p.av.data(), p.bv.data(), p.k0.data(), p.n0.data(), p.k1.data(), p.n1.data(),
                            p.gv.data(), p.rho.data(), net_null ? nullptr : &p.na, net_null ? nullptr : &p.nb, msg, cap);
}

// The sizing functions of the two fits against the sums the four drivers wrote out before they shared one loop (copied here
// as the expected values), and the bump allocator against a carving in the loop's order.
static void sizing_checks()
{
    for (size_t N : {1, 3, 130}) for (size_t B : {1, 3}) for (size_t T : {50, 700}) for (size_t Tb : {(size_t)16, (size_t)112, T})
    for (size_t L : {0, 1, 7}) for (size_t KB : {0, 1, 8}) for (size_t bm : {128, 160}) for (size_t splits : {1, 3}) {
        if (Tb > T) continue;
        const size_t NN = N * N, K = N * B;
        const bool streamed = L > 0, sb = KB > 0;
        // VB: one window of T bins, its own row blocks and splits (no streamed mode)
        const size_t row_blocks = (T + bm - 1) / bm;
        const disc_vb_dims vb{N, B, T, row_blocks, splits, false, 0};
        const size_t need_vb = 8 * (K * N + N + N + N + NN + NN + NN * B + T * N + (size_t)row_blocks * N + (size_t)splits * K * N);
        const size_t need_netvb = 8 * (netvb_param_doubles(N, B) + T * N + (size_t)row_blocks * N + (size_t)splits * K * N +
                                       (sb ? sbmvb_param_doubles(N, KB, false) : 0));
        EXPECT(8 * dense_vb_reserve_doubles(vb) == need_vb);
        EXPECT(8 * netvb_reserve_doubles(vb, sb ? sbmvb_param_doubles(N, KB, false) : 0) == need_netvb);
        // SVI: blocks of Tb bins, the caps of a whole block
        const size_t max_row_blocks = (Tb + 127) / 128, max_splits = splits;
        const disc_vb_dims svi{N, B, Tb, max_row_blocks, max_splits, true, L};
        const size_t need_svi = 8 * (K * N + N + N + N + NN + NN + NN * B + 2 * (size_t)Tb * N + max_row_blocks * N + (size_t)max_splits * K * N +
                                     (streamed ? (size_t)Tb * K + L * B : 0));
        const size_t need_netsvi = 8 * (netvb_param_doubles(N, B) + 2 * (size_t)Tb * N + max_row_blocks * N + (size_t)max_splits * K * N +
                                        (streamed ? (size_t)Tb * K + L * B : 0) + (sb ? sbmvb_param_doubles(N, KB, true) : 0));
        EXPECT(8 * dense_vb_reserve_doubles(svi) == need_svi);
        EXPECT(8 * netvb_reserve_doubles(svi, sb ? sbmvb_param_doubles(N, KB, true) : 0) == need_netsvi);
        // a carving in the loop's order takes what the sizing says: the dense fit, then the network fit with its block model
        const size_t blk = sb ? sbmvb_param_doubles(N, KB, true) : 0;
        std::vector<double> buf(netvb_reserve_doubles(svi, blk) + 1);
        auto window = [&](vb_bump &m) {
            m.take(Tb * N); m.take(Tb * N); m.take(max_row_blocks * N); m.take(max_splits * K * N);       // D, R, partials, slabs
            m.take(streamed ? Tb * K : 0); m.take(L * B);                                                   // image, basis
        };
        vb_bump dense(buf.data());
        dense.take(K * N); dense.take(3 * N); dense.take(2 * NN); dense.take(NN * B);                     // E; e0, αv, βv; κv, νv; γv
        window(dense);
        EXPECT(dense.used() == dense_vb_reserve_doubles(svi));
        vb_bump net(buf.data());
        net.take(K * N); net.take(3 * N); net.take(4 * NN); net.take(NN * B); net.take(NN);               // ... κv0, νv0, κv1, νv1; γv; ρv
        net.take(2); net.take(2 * netvb_link_blocks(N));                                                   // network scalars, ρv partials
        window(net);
        if (sb) {                                      // the block model: state, hats, D, four tables, Eπ, m·D, U1, U0, ρ̂v
            const size_t NK = N * KB, KK = KB * KB;
            for (int twice = 0; twice < 2; ++twice) { net.take(NK); net.take(KK); net.take(KK); net.take(KB); }
            net.take(KK); net.take(4 * KK); net.take(KB); net.take(3 * NK); net.take(NN);
        }
        EXPECT(net.used() == netvb_reserve_doubles(svi, blk) && net.used() < buf.size());
    }
}

static int sched(const char *what, const svi_request &rq, int32_t n_steps, int64_t T, bool base, bool trials, bool conv, svi_schedule *sc, char *msg)
{
    return svi_check_schedule(what, rq, n_steps, T, base, trials, conv, sc, msg, 256);
}

// every schedule error: the status and the message the SVI drivers gave, with the caller's prefix
static void schedule_checks()
{
    char msg[256];
    svi_schedule sc;
    const double phi[8] = {0};
    const int32_t blocks_ok[3] = {0, 6, 1}, blocks_bad[3] = {0, 7, 1};
    const svi_request ok{112, 1.0, 0.6, 7, 0, nullptr, nullptr, 0, 0};
    for (const char *what : {"svi", "netsvi", "sbmsvi"}) {
        const std::string w(what);
        auto is = [&](int rc, int want, const std::string &text) { return rc == want && w + ": " + text == msg; };
        EXPECT(sched(what, ok, 3, 700, false, false, true, &sc, msg) == NETVB_OK && msg[0] == 0 && sc.Tb == 112 && sc.nb == 7 && !sc.streamed);
        svi_request r = ok;
        r.batch_bins = 1000;                                                     // >= T: one block, any size
        EXPECT(sched(what, r, 1, 700, false, false, true, &sc, msg) == NETVB_OK && sc.Tb == 700 && sc.nb == 1);
        r = ok; r.blocks = blocks_ok;
        EXPECT(sched(what, r, 3, 700, false, false, true, &sc, msg) == NETVB_OK);
        r = ok; r.phi = phi; r.n_lags = 7; r.n_basis = 3;                        // streamed needs no resident image
        EXPECT(sched(what, r, 3, 700, false, false, false, &sc, msg) == NETVB_OK && sc.streamed);
        EXPECT(is(sched(what, ok, 0, 700, false, false, true, &sc, msg), NETVB_EINVAL, "n_steps must be >= 1 and step0 >= 0"));
        r = ok; r.step0 = -1;
        EXPECT(is(sched(what, r, 1, 700, false, false, true, &sc, msg), NETVB_EINVAL, "n_steps must be >= 1 and step0 >= 0"));
        r = ok; r.delay = -0.5;
        EXPECT(is(sched(what, r, 1, 700, false, false, true, &sc, msg), NETVB_EINVAL, "delay must be >= 0"));
        r = ok; r.delay = std::numeric_limits<double>::quiet_NaN();
        EXPECT(is(sched(what, r, 1, 700, false, false, true, &sc, msg), NETVB_EINVAL, "delay must be >= 0"));
        for (double f : {0.5, 1.5, std::numeric_limits<double>::quiet_NaN()}) {
            r = ok; r.forgetting = f;
            EXPECT(is(sched(what, r, 1, 700, false, false, true, &sc, msg), NETVB_EINVAL, "forgetting must lie in (0.5, 1]"));
        }
        for (int64_t bb : {0, 8, 100}) {
            r = ok; r.batch_bins = bb;
            EXPECT(is(sched(what, r, 1, 700, false, false, true, &sc, msg), NETVB_EINVAL,
                      "batch_bins = " + std::to_string(bb) + " must be a multiple of 16 (>= 16), or >= the 700 bins of the data"));
        }
        r = ok; r.blocks = blocks_bad;
        EXPECT(is(sched(what, r, 3, 700, false, false, true, &sc, msg), NETVB_EINVAL, "blocks[1] = 7 is outside [0, 7)"));
        EXPECT(is(sched(what, ok, 1, 700, true, false, true, &sc, msg), NETVB_ENOTIMPL, "defined for DiscreteHomogeneousProcess baselines only"));
        r = ok; r.phi = phi; r.n_lags = 7; r.n_basis = 3;
        EXPECT(is(sched(what, r, 1, 700, false, true, true, &sc, msg), NETVB_ENOTIMPL,
                  "the streamed mode convolves across the boundaries of the dataset's trials; convolve the dataset and use the resident mode"));
        r.n_lags = 0;
        EXPECT(is(sched(what, r, 1, 700, false, false, true, &sc, msg), NETVB_EINVAL, "the streamed mode needs n_lags >= 1 and n_basis >= 1"));
        EXPECT(is(sched(what, ok, 1, 700, false, false, false, &sc, msg), NETVB_EINVAL,
                  "convolve(process, data) must run first, or pass the basis for the streamed mode"));
        r.n_lags = 800; r.n_basis = 9;                                           // 8 (256 + 800 + 800·16) bytes > 64 KiB
        EXPECT(is(sched(what, r, 1, 700, false, false, true, &sc, msg), NETVB_ENOTIMPL, "nlags * nbasis = 800 * 9 exceeds the LDS budget"));
        r.n_basis = 3;                                                           // 8 (256 + 800 + 800·8) bytes fit 
        EXPECT(sched(what, r, 1, 700, false, false, true, &sc, msg) == NETVB_OK);
    }
    EXPECT(svi_window_lds_bytes(7, 3) == 8 * (256 + 7 + 7 * 8));
}

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const netvb_priors ok{1.0, 1.0, 0.5, 20.0, 2.0, 1.5, 1.0, 1, 1.5, 2.5};
    char msg[256];
    for (int64_t N : {1, 3, 130}) {
        for (int64_t B : {1, 3}) {
            params p((size_t)N, (size_t)B);
            EXPECT(run(ok, 1.0, N, B, 1, p, msg, sizeof msg) == NETVB_OK && msg[0] == 0);
            netvb_priors dense = ok;
            dense.net_kind = 0;
            p.rho.assign(p.rho.size(), 7.0);                        // a dense network ignores rho_v and needs no network pointers
            EXPECT(run(dense, 1.0, N, B, 1, p, msg, sizeof msg, true) == NETVB_OK);
            EXPECT(run(ok, 1.0, N, B, 1, p, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "rho_v"));
            p.rho.assign(p.rho.size(), 0.0);
            p.rho.back() = 1.0;                                     // the closed ends are allowed
            EXPECT(run(ok, 1.0, N, B, 1, p, msg, sizeof msg) == NETVB_OK);
            p.rho.back() = nan;
            EXPECT(run(ok, 1.0, N, B, 1, p, msg, sizeof msg) == NETVB_EINVAL);
            p.rho.back() = 0.5;
            EXPECT(run(ok, 1.0, N, B, 1, p, msg, sizeof msg, true) == NETVB_EINVAL && std::strstr(msg, "net_alpha_v"));
            p.k1.back() = 0.0;
            EXPECT(run(ok, 1.0, N, B, 1, p, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "kappa_v"));
            p.k1.back() = 2.0;
            p.n0.front() = -1.0;
            EXPECT(run(ok, 1.0, N, B, 1, p, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "nu_v"));
            p.n0.front() = 20.0;
            p.gv.back() = nan;
            EXPECT(run(ok, 1.0, N, B, 1, p, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "gamma_v"));
            p.gv.back() = 1.0;
            p.bv.back() = 0.0;
            EXPECT(run(ok, 1.0, N, B, 1, p, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "beta_v"));
            p.bv.back() = 2.0;
            p.na = 0.0;
            EXPECT(run(ok, 1.0, N, B, 1, p, msg, sizeof msg) == NETVB_EINVAL);
            p.na = 1.5;
            EXPECT(run(ok, 1.0, N, B, 0, p, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "n_steps"));
            EXPECT(run(ok, 0.0, N, B, 1, p, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "dt"));
            for (int kind : {-1, 2, 7}) {
                netvb_priors bad = ok;
                bad.net_kind = kind;
                EXPECT(run(bad, 1.0, N, B, 1, p, msg, sizeof msg) == NETVB_ENOTIMPL && std::strstr(msg, "net_kind"));
            }
            for (double v : {0.0, -2.0, nan, inf}) {
                netvb_priors bad = ok;
                bad.nu0 = v;
                EXPECT(run(bad, 1.0, N, B, 1, p, msg, sizeof msg) == NETVB_EINVAL && std::strstr(msg, "weight priors"));
                bad = ok;
                bad.kappa1 = v;
                EXPECT(run(bad, 1.0, N, B, 1, p, msg, sizeof msg) == NETVB_EINVAL);
            }
            char tiny[8];                                           // a short message buffer is cut, not overrun
            p.rho.front() = 2.0;
            EXPECT(run(ok, 1.0, N, B, 1, p, tiny, sizeof tiny) == NETVB_EINVAL && std::strlen(tiny) == sizeof tiny - 1);
            // the sizing: every buffer the run carves fits, in the order it carves them
            const size_t n = (size_t)N, b = (size_t)B, nn = n * n;
            const size_t want = n * b * n + 3 * n + 4 * nn + nn * b + nn + 2 + 2 * ((nn + 255) / 256);
            EXPECT(netvb_param_doubles(n, b) == want);
            EXPECT(netvb_link_blocks(n) * 256 >= nn && (netvb_link_blocks(n) - 1) * 256 < nn);
        }
    }
    sizing_checks();
    schedule_checks();
    EXPECT(netvb_link_blocks(130) == 67);
    const double pl = netvb_prior_logit(ok);
    EXPECT(std::fabs(pl - ((2.0 * std::log(1.5) - std::lgamma(2.0)) - (0.5 * std::log(20.0) - std::lgamma(0.5)))) < 1e-15);
    netvb_priors sym = ok;
    sym.kappa1 = sym.kappa0; sym.nu1 = sym.nu0;
    EXPECT(netvb_prior_logit(sym) == 0.0);
    std::printf(failures ? "%d check(s) failed\n" : "netvb host checks passed\n", failures);
    return failures ? 1 : 0;
}
