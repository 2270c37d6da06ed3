"""The shared exit of the child-slice kernels (csrc/cont_slices.hip: sl_exit_sums), restated in numpy: Σ log λ of a
wave as ONE logarithm of the product of its 64 mantissas plus the integer sum of their exponents times ln 2, the waves' values
added in wave order.  No GPU.

Steps, in the kernel's order: frexp of every rate (mantissa in [0.5, 1)); the mantissas multiplied pairwise -- lanes i and i^1, the
pairs of a quad, the quads of a group of 8, the groups of a row of 16 (the DPP steps) -- then the four rows in row order; the
exponents added as integers; frexp of the product; log(mantissa) + exponent · ln 2; eight waves make a workgroup.

References: math.fsum of the 64 logarithms, whose own error (one ulp of every log r) is added to the bound; and the exact value,
the logarithm (mpmath, 40 digits) of the exact integer product of the mantissas, which is held to the formation's bound alone.

The bound, per wave, in units of u = 2^-53:  64 u for the product (63 multiplications of relative error u each, |Δ log P| =
63 u (1 + O(u)); frexp is exact), u for the logarithm of a mantissa (|log m| < 0.7: one ulp is at most u), |E| u / 2 for the
constant ln 2 (rounded to nearest in [0.5, 1)) and u |E ln 2| for the product E · ln 2, u |value| for the last addition.  Per
workgroup: the waves' bounds and u times every partial sum of the seven additions."""
import math

import numpy as np

U = 2.0 ** -53
LN2 = 6.93147180559945286e-01
WAVES = 10_000
NW = 8


def formation(rates):
    """rates [W, 64] -> (value, exponent) per wave."""
    m, e = np.frexp(rates)
    p = m.reshape(-1, 4, 2, 2, 2, 2)                     # row, group of 8, quad, pair, lane
    for _ in range(4):
        p = p[..., 0] * p[..., 1]
    r = ((p[:, 0] * p[:, 1]) * p[:, 2]) * p[:, 3]
    assert np.all(r >= 2.0 ** -64)
    mant, ex = np.frexp(r)
    E = e.sum(axis=1, dtype=np.int64) + ex
    return np.log(mant) + E.astype(np.float64) * LN2, E


def wave_bound(value, E):
    return U * (64.0 + 1.0 + 0.5 * np.abs(E) + np.abs(E * LN2) + np.abs(value))


def exact_log_of_product(rates):
    import mpmath
    mpmath.mp.dps = 40
    out = []
    for row in rates:
        num, shift = 1, 0
        for x in row:
            m, e = math.frexp(x)
            num *= int(m * 2.0 ** 53)                    # (exact: a double's 53 bits)
            shift += e - 53
        out.append(mpmath.log(mpmath.mpf(num)) + shift * mpmath.log(2))
    return out


def test_one_logarithm_per_wave():
    rng = np.random.default_rng(20260)
    rates = 10.0 ** rng.uniform(-300.0, 300.0, (WAVES, 64))             # 600 orders of magnitude
    got, E = formation(rates)
    bound = wave_bound(got, E)
    logs = np.log(rates)
    ref = np.array([math.fsum(row) for row in logs])
    ref_err = np.spacing(np.abs(logs)).sum(axis=1)                      # one ulp per logarithm of the reference
    worst_fsum = np.max(np.abs(got - ref) / (bound + ref_err))
    import mpmath
    exact = exact_log_of_product(rates)
    err = np.array([float(abs(mpmath.mpf(float(g)) - x)) for g, x in zip(got, exact)])
    worst_exact = np.max(err / bound)
    print(f"waves {WAVES}: error / bound, against fsum {worst_fsum:.3f}, against the exact value {worst_exact:.3f}; "
          f"largest error {err.max():.3e} ({np.max(err / np.abs(got)):.2e} relative)")
    assert worst_fsum <= 1.0 and worst_exact <= 1.0
    # a workgroup: the eight waves' values added in wave order
    blocks = got.reshape(-1, NW)
    part = np.cumsum(blocks, axis=1)                                    # (numpy's cumsum adds sequentially)
    block_bound = bound.reshape(-1, NW).sum(axis=1) + U * np.abs(part[:, 1:]).sum(axis=1)
    exact_b = [sum(exact[NW * b:NW * b + NW]) for b in range(len(blocks))]
    err_b = np.array([float(abs(mpmath.mpf(float(g)) - x)) for g, x in zip(part[:, -1], exact_b)])
    print(f"workgroups of {NW} waves: error / bound {np.max(err_b / block_bound):.3f}")
    assert np.all(err_b <= block_bound)


def test_edges_of_the_formation():
    """A lane without a child is {1.0, 0}: frexp(1.0) = {0.5, 1}, and a whole wave of them gives exactly 0.  λ = 0 gives -inf."""
    ones = np.ones((1, 64))
    got, E = formation(ones)
    assert got[0] == 0.0 and math.log(0.5) + LN2 == 0.0
    rates = np.full((1, 64), 3.0)
    rates[0, 17] = 0.0
    m, e = np.frexp(rates)
    assert m[0, 17] == 0.0 and np.prod(m) == 0.0
    with np.errstate(divide="ignore"):
        assert np.log(np.prod(m)) + e.sum() * LN2 == -np.inf
    # what a plain product would do with the exponents left in: 64 rates of 1e-300 underflow, of 1e+300 overflow
    with np.errstate(over="ignore", under="ignore"):
        assert np.prod(np.full(64, 1e-300)) == 0.0 and np.prod(np.full(64, 1e300)) == np.inf
    for r in (1e-300, 1e300):
        got, E = formation(np.full((1, 64), r))
        assert abs(got[0] - 64 * math.log(r)) <= wave_bound(got, E)[0] + 64 * np.spacing(abs(math.log(r)))
