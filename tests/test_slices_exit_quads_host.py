"""The shared exit of the child-slice kernels after its wave-wide product tree was cut back to the quad steps (csrc/cont_slices.hip:
sl_exit_sums; DESIGN 3.1d, "The exit by quads"), restated in numpy.  No GPU.

Steps, in the kernel's order.  A lane holds a mantissa in [0.5, 1) and an integer exponent (frexp of its rate; a lane without a
child holds {1.0, 0} in a wave that had no slice, {0.5, 1} in one that had).  Two DPP steps: lanes i and i^1 multiply their
mantissas, then the two pairs of a quad multiply theirs; the exponents are added the same way.  The lanes with (lane & 3) == 0 park
the 16 quad products and 16 quad exponent sums of (model, wave).  One lane of the first wave multiplies the 16 products in lane order
((q0·q1)·q2 ...), adds the 16 exponents, takes frexp of the product once, and forms log(mantissa) + exponent · ln 2: one logarithm
per (model, wave).  Thread 0 adds a model's values wave by wave.

The bound is the one tests/test_slices_epilogue_host.py derives for the tree that ran all four DPP steps and multiplied the four rows,
restated for this order; u = 2^-53.  A quad product is two pair products and their product: 3 multiplications per quad, 48 in the
wave; the 16 quad products take 15 more: 63 multiplications, as before.  Every one has a relative error of at most u, whatever the
association, so |Δ log P| <= 63 u (1 + O(u)), counted as 64 u.  No intermediate can underflow or leave the normal range: a mantissa is
>= 1/2, a quad product >= 2^-4, the product of sixteen >= 2^-64, and frexp is exact.  Then u for the logarithm of a mantissa
(|log m| < 0.7: one ulp is at most u), |E| u / 2 for the constant ln 2 (rounded to nearest in [0.5, 1)), u |E ln 2| for the product
E · ln 2 and u |value| for the last addition.  Per workgroup: the waves' bounds and u times every partial sum of the NW - 1 additions.

References: the exact value, the logarithm (mpmath, 40 digits) of the exact integer product of the mantissas, held to the formation's
bound alone; and math.fsum of the 64 logarithms, whose own error (one ulp of every logarithm) is added to the bound.

Planted mistakes, each of which the comparison must catch: a quad's exponent sum dropped, the 16 products taken from the other
model's row, and the {0.5, 1} convention of a wave without children broken."""
import math

import numpy as np

U = 2.0 ** -53
LN2 = 6.93147180559945286e-01
WAVES = 4000
NW = 8


def lanes_of(rates, had_slice=True):
    """rates [.., 64], NaN = a lane without a child -> (mantissa, exponent) as the row loop leaves them."""
    empty = np.isnan(rates)
    m, e = np.frexp(np.where(empty, 1.0, rates))
    if not had_slice:                                                   # {1.0, 0}: never renormalised
        m, e = np.where(empty, 1.0, m), np.where(empty, 0, e)
    return m, e.astype(np.int64)


def formation(mant, ex, mistake=None):
    """mant, ex [S, W, 64] -> (value [S, W], exponent [S, W]): sl_exit_sums for S models and W waves."""
    S, W, _ = mant.shape
    q = mant.reshape(S, W, 16, 2, 2)                                    # quad, pair, lane
    q = q[..., 0] * q[..., 1]                                           # lanes i and i^1
    q = q[..., 0] * q[..., 1]                                           # the two pairs of a quad
    qe = ex.reshape(S, W, 16, 4).sum(axis=3)
    assert np.all((q >= 2.0 ** -4) | (q == 0.0) | np.isnan(q))
    if mistake == "quad exponent dropped":
        qe = qe.copy()
        qe[:, :, 5] = 0
    if mistake == "other model's row":
        q = q[::-1]
    r = q[..., 0]
    for i in range(1, 16):                                              # lane q of the first wave: in lane order
        r = r * q[..., i]
    assert np.all((r >= 2.0 ** -64) | (r == 0.0) | np.isnan(r))
    m, e = np.frexp(r)
    E = qe.sum(axis=2) + e
    if mistake == "empty wave":                                         # {0.5, 0}: the renormalisation's exponent forgotten
        E = qe.sum(axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(m) + E.astype(np.float64) * LN2, E


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
            num *= int(m * 2.0 ** 53)                                   # (exact: a double's 53 bits)
            shift += e - 53
        out.append(mpmath.log(mpmath.mpf(num)) + shift * mpmath.log(2))
    return out


def world():
    """Two models' rates over 600 orders of magnitude, [2, WAVES, 64], with their exact values; made once."""
    if not hasattr(world, "v"):
        rng = np.random.default_rng(20261)
        rates = 10.0 ** rng.uniform(-300.0, 300.0, (2, WAVES, 64))
        exact = [exact_log_of_product(rates[s]) for s in range(2)]
        world.v = (rates, exact)
    return world.v


def errors(got, exact):
    import mpmath
    return np.array([[float(abs(mpmath.mpf(float(g)) - x)) for g, x in zip(got[s], exact[s])] for s in range(got.shape[0])])


def test_quads_then_sixteen_in_lane_order():
    rates, exact = world()
    got, E = formation(*lanes_of(rates))
    bound = wave_bound(got, E)
    err = errors(got, exact)
    logs = np.log(rates)
    ref = np.array([[math.fsum(row) for row in logs[s]] for s in range(2)])
    ref_err = np.spacing(np.abs(logs)).sum(axis=2)
    worst_fsum = np.max(np.abs(got - ref) / (bound + ref_err))
    print(f"waves 2 x {WAVES}: error / bound, against the exact value {np.max(err / bound):.3f}, against fsum {worst_fsum:.3f}; "
          f"largest error {err.max():.3e} ({np.max(err / np.abs(got)):.2e} relative)")
    assert np.all(err <= bound) and worst_fsum <= 1.0
    # a workgroup: a model's waves added in wave order
    blocks = got.reshape(2, -1, NW)
    part = np.cumsum(blocks, axis=2)                                    # (numpy's cumsum adds sequentially)
    block_bound = bound.reshape(2, -1, NW).sum(axis=2) + U * np.abs(part[:, :, 1:]).sum(axis=2)
    import mpmath
    for s in range(2):
        exact_b = [sum(exact[s][NW * b:NW * b + NW]) for b in range(blocks.shape[1])]
        err_b = np.array([float(abs(mpmath.mpf(float(g)) - x)) for g, x in zip(part[s, :, -1], exact_b)])
        assert np.all(err_b <= block_bound[s]), s
    # against the formation it replaces (four DPP steps, then the four rows): both within the bound of the exact value, so within
    # twice the bound of each other -- what `bench.py --dump-outputs` may move by against the parent
    m, e = lanes_of(rates)
    p = m.reshape(2, WAVES, 4, 2, 2, 2, 2)
    for _ in range(4):
        p = p[..., 0] * p[..., 1]
    old_m, old_e = np.frexp(((p[..., 0] * p[..., 1]) * p[..., 2]) * p[..., 3])
    old = np.log(old_m) + (e.sum(axis=2) + old_e).astype(np.float64) * LN2
    moved = np.abs(old - got)
    print(f"against the four-step tree: {np.count_nonzero(moved)} of {moved.size} waves differ, at most {np.max(moved / bound):.3f} of the bound")
    assert np.all(moved <= 2.0 * bound)


def test_planted_mistakes_are_caught():
    rates, exact = world()
    m, e = lanes_of(rates)
    for mistake in ("quad exponent dropped", "other model's row"):
        got, E = formation(m, e, mistake)
        err = errors(got[:, :50], [x[:50] for x in exact])
        caught = np.count_nonzero(err > wave_bound(got, E)[:, :50])
        print(f"{mistake}: outside the bound in {caught} of {err.size} waves")
        assert caught >= err.size - 2, mistake                          # (a dropped exponent sum of exactly 0 changes nothing)
    # the rows swapped must also show when the two models' exponents happen to agree: same exponents, other mantissas
    got, E = formation(m, np.broadcast_to(e[:1], e.shape), "other model's row")
    right, _ = formation(m, np.broadcast_to(e[:1], e.shape))
    assert np.count_nonzero(got != right) > 0.99 * got.size
    # a wave without children
    none = np.full((1, 1, 64), np.nan)
    for had_slice in (False, True):
        got, E = formation(*lanes_of(none, had_slice))
        assert got[0, 0] == 0.0, (had_slice, got)
    got, E = formation(*lanes_of(none, False), "empty wave")
    assert got[0, 0] != 0.0 and got[0, 0] == math.log(0.5)


def test_edges_of_the_formation():
    """A wave without a slice: every lane {1.0, 0}, the product 1.0 = {0.5, 1}, and log 0.5 + ln 2 is exactly 0.  Part-filled slices:
    5, 4 and 1 children (a quad partly filled, exactly one quad, one lane of one quad) give the logarithm of those children alone.
    λ = 0 in a lane with (lane & 3) != 0 reaches the result through the quad step only: -inf; λ < 0 arrives as a NaN mantissa."""
    assert math.log(0.5) + LN2 == 0.0
    rng = np.random.default_rng(20262)
    for n in (5, 4, 1):
        rates = np.full((1, 1, 64), np.nan)
        rates[0, 0, :n] = 10.0 ** rng.uniform(-300.0, 300.0, n)
        want = math.fsum(np.log(rates[0, 0, :n]))
        for had_slice in (False, True):
            got, E = formation(*lanes_of(rates, had_slice))
            assert abs(got[0, 0] - want) <= wave_bound(got, E)[0, 0] + np.spacing(np.abs(np.log(rates[0, 0, :n]))).sum(), (n, had_slice)
    rates = np.full((2, 1, 64), 3.0)
    rates[0, 0, 18] = 0.0                                               # lane 18: (lane & 3) == 2
    m, e = lanes_of(rates)
    got, _ = formation(m, e)
    assert got[0, 0] == -np.inf and np.isfinite(got[1, 0])
    m[0, 0, 18] = np.nan                                                # what the row loop leaves for λ < 0
    got, _ = formation(m, e)
    assert np.isnan(got[0, 0]) and np.isfinite(got[1, 0])
    # 64 rates of 1e-300 or 1e+300: a plain product would underflow or overflow
    for r in (1e-300, 1e300):
        got, E = formation(*lanes_of(np.full((1, 1, 64), r)))
        assert abs(got[0, 0] - 64 * math.log(r)) <= wave_bound(got, E)[0, 0] + 64 * np.spacing(abs(math.log(r)))
