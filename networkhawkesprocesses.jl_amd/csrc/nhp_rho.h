// The device-side draw of a Bernoulli network's link probability, shared by the two device-resident chains.
#pragma once
#include "nhp_rng.h"

// BernoulliNetworkModel's resample!(network, A) (src/networks.jl:70-78) on the device: ρ ~ Beta(α + ΣA, β + N² - ΣA) as
// X / (X + Y), X ~ Gamma(α + ΣA), Y ~ Gamma(β + N² - ΣA), Philox-keyed (seed, step).  state = {ρ, Σρ, Σρ², ΣA}: the scalars
// a device-resident model keeps for its network, continuous (cont_adjacency.hip) or discrete (disc_chain.hip) -- one kernel
// for both, so the two chains draw the same ρ from the same link count.
static __global__ void k_rho_draw(double *__restrict__ state, double alpha, double beta, double nn, uint64_t seed, uint64_t step)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double links = state[3];
    const double x = dev_gamma(alpha + links, 1.0, seed ^ 0x3F84D5B5B5470917ull, step, 0);
    const double y = dev_gamma(beta + nn - links, 1.0, seed ^ 0x3F84D5B5B5470917ull, step, 1);
    state[0] = x / (x + y);
}
