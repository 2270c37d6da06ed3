"""The slice kernels' pair term on the host (csrc/nhp_math.h: nhp_exp_term_fast / nhp_exp_term_slow).

Both sequences are restated operation by operation -- every fma exact (rational arithmetic, rounded once), the biased table of
2^(j/64), the integer add into the high dword, the saturating conversion and ldexp of the slow path -- on the table READ FROM
THE HEADER, and held to
  * exp in 200-bit arithmetic: 5e-16 relative per term (what the issue of this change sets);
  * each other: bit for bit wherever |cx·v| is inside the limit and the result is a normal number;
  * a restatement of the helper they replace (nhp_exp_neg_tab_scaled on 64 entries): never further than that helper's own
    error, 8e-14 + 3e-16 relative; below the normal range within that and one unit of 2^-1074, and 0 where it gives 0.
Ranges: θ·Δtmax log-uniform in [1e-6, 700], 37-bit delays (the headline's records), the delay's extremes 1 and 2^37 - 1.
Which path an item takes (cont_slices.hip: sl_term_outside against sl_term_limit) is restated too: past the limit, past 2^31
and non-finite rates must come out `outside`.  Two planted mistakes must each fail the comparison."""
import math
import os
import re
import struct
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "networkhawkesprocesses.jl_amd", "csrc", "nhp_math.h")

LOG = 6
T = 1 << LOG
MAGIC = 6755399441055744.0                                    # 1.5·2^52
DBITS = 37
LIMIT = 1015.625 * T                                          # nhp_exp_term_limit
TOL = 5e-16


def header_table(name):
    src = open(HEADER).read()
    m = re.search(r"const double " + name + r"\[64\] = \{(.*?)\};", src, re.S)
    return [float.fromhex(x) for x in re.findall(r"0x1\.[0-9a-f]+p\+0", m.group(1))]


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b & 0xFFFFFFFFFFFFFFFF))[0]


def fma(a, b, c):
    """One rounding of the exact a·b + c."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return a * b + c                                       # (the sign of an exact zero, as IEEE has it)
    try:
        return float(r)
    except OverflowError:
        return math.inf if r > 0 else -math.inf


def sat_i32(x):
    """v_cvt_i32_f64: truncates, saturates, NaN -> 0."""
    if x != x:
        return 0
    return int(max(-2.0 ** 31, min(2.0 ** 31 - 1, x)))


D1, D2, D3, D4, D5 = (float.fromhex("0x1.62e42fefa39efp-7"), float.fromhex("0x1.ebfbdff82c58fp-15"), float.fromhex("0x1.c6b08d704a0c0p-23"),
                      float.fromhex("0x1.3b2ab6fba4e77p-31"), float.fromhex("0x1.5d87fe78a6731p-40"))


def poly5(u):
    """(ln2/64)^i / i!, Horner by fma, the last step a multiplication: both helpers and the present one."""
    p = fma(D5, u, D4)
    p = fma(p, u, D3)
    p = fma(p, u, D2)
    p = fma(p, u, D1)
    return p * u


def biased(tab):
    out = []
    for j, e in enumerate(tab):
        b = bits(e)
        hi = ((b >> 32) - (j << (20 - LOG))) & 0xFFFFFFFF
        out.append((hi << 32) | (b & 0xFFFFFFFF))
    return out


def add_hi(entry_bits, k):
    hi = ((entry_bits >> 32) + (k << (20 - LOG))) & 0xFFFFFFFF
    return from_bits((hi << 32) | (entry_bits & 0xFFFFFFFF))


def reduce_(cx, v):
    km = fma(cx, v, MAGIC)
    kf = km - MAGIC
    u = fma(cx, v, -kf)
    return km, kf, u


def term_fast(cx, v, tabb):
    km, kf, u = reduce_(cx, v)
    k = bits(km) & 0xFFFFFFFF                                  # the low dword, as it stands
    ts = add_hi(tabb[k & (T - 1)], k)
    return fma(ts, poly5(u), ts)


def term_slow(cx, v, tabb, low_dword_k=False):
    km, kf, u = reduce_(cx, v)
    if low_dword_k:                                            # (planted mistake)
        k = bits(km) & 0xFFFFFFFF
        k = k - (1 << 32) if k >= 1 << 31 else k
    else:
        k = sat_i32(kf)
    if 2.0 ** 31 <= abs(kf) < math.inf:                        # k is saturated: the result is 0 or inf whatever u is, and u is the
        u = 0.0                                                #  product's rounding error once |cx·v| passes 2^106
    j = k & (T - 1)
    t1 = add_hi(tabb[j], j)
    r = fma(t1, poly5(u), t1)
    if r != r or math.isinf(r):
        return r
    try:
        return math.ldexp(r, k >> LOG)
    except OverflowError:
        return math.copysign(math.inf, r)


def term_present(cx64, v, tab64):
    """nhp_exp_neg_tab_scaled(cx64 * v): the helper the new ones replace."""
    t = cx64 * v
    if t != t:
        return t
    kf = float(round(t)) if math.isfinite(t) else t            # round(): to nearest, ties to even (v_rndne_f64)
    u = t - kf
    k = sat_i32(kf)
    tb = tab64[k & 63]
    r = fma(tb, poly5(u), tb)
    if r != r:
        return r
    return math.ldexp(r, k >> 6)


def outside(cx):
    """sl_term_outside(cx, sl_term_limit(dbits))."""
    return not (abs(cx) <= math.ldexp(LIMIT, -DBITS))


def column_entry(theta_dtmax, scale):
    """-((θ·unit)·scale) with Δtmax = 1: the head's three roundings."""
    unit = math.ldexp(1.0, -DBITS)
    return -((theta_dtmax * unit) * scale)


K64 = 92.33248261689366                                      # 64 / ln 2, as the kernels' heads write it


def exact(cx, v):
    mp.mp.prec = 200
    return mp.exp(mp.mpf(cx) * mp.mpf(v) * mp.log(2) / T)


def relerr(x, ref):
    return float(abs((mp.mpf(x) - ref) / ref))


@pytest.fixture(scope="module")
def tables():
    t64 = header_table("nhp_exp2_64")
    assert len(t64) == 64
    return t64, biased(t64)


@pytest.fixture(scope="module")
def terms():
    """(θ·Δtmax, delay) pairs: log-uniform arguments, uniform 37-bit delays, the delay's ends."""
    rng = np.random.default_rng(18)
    n = 4000
    th = np.exp(rng.uniform(math.log(1e-6), math.log(700.0), n))
    v = rng.integers(1, 2 ** DBITS, n).astype(np.float64)
    v[:200] = 2.0 ** DBITS - 1
    v[200:300] = 1.0
    th[:50] = 700.0
    return [(float(a), float(b)) for a, b in zip(th, v)]


def test_tables_in_the_header(tables):
    """Correctly rounded 2^(j/64); un-biasing gives the entry back, and adding k << 14 scales it by 2^(k >> 6) exactly."""
    t64, tabb = tables
    mp.mp.prec = 200
    for j in range(64):
        want = mp.mpf(2) ** (mp.mpf(j) / 64)
        assert abs(mp.mpf(t64[j]) - want) <= mp.mpf(2) ** -53, j       # half an ulp of [1, 2)
    for j in (0, 1, 37, 63):
        assert add_hi(tabb[j], j) == t64[j]
        for n in (-1016, -3, 0, 5, 1015):
            assert add_hi(tabb[j], (n * T + j) & 0xFFFFFFFF) == math.ldexp(t64[j], n)


def compare(tables, terms, tabb=None, low_dword_k=False, extremes=True):
    """The whole comparison; the planted mistakes go through it too.  Returns the worst figures."""
    t64, good = tables
    tabb = good if tabb is None else tabb
    worst_new = worst_old = worst_move = 0.0
    moved = 0
    for th, v in terms:
        cx = column_entry(th, K64)
        assert not outside(cx)
        f = term_fast(cx, v, tabb)
        s = term_slow(cx, v, tabb, low_dword_k)
        assert f == s, (th, v, f, s)
        ref = exact(cx, v)
        e_new = relerr(f, ref)
        old = term_present(cx, v, t64)
        e_old = relerr(old, ref)
        worst_new, worst_old = max(worst_new, e_new), max(worst_old, e_old)
        assert e_new < TOL, (th, v, e_new)
        move = abs(f - old) / old
        worst_move = max(worst_move, move)
        moved += f != old
        assert move <= 8e-14 + 3e-16, (th, v, move)
    if extremes:
        vmax = 2.0 ** DBITS - 1
        # at the limit itself both paths are valid and agree (k = -65000 at the largest delay: exponent -1016)
        cx = -math.ldexp(LIMIT, -DBITS)
        assert not outside(cx) and outside(math.nextafter(cx, -math.inf))
        for v in (vmax, vmax - 1, 2.0 ** 36, 1.0):
            f, s = term_fast(cx, v, tabb), term_slow(cx, v, tabb, low_dword_k)
            assert f == s and relerr(f, exact(cx, v)) < TOL
        assert math.frexp(term_fast(cx, vmax, tabb))[1] - 1 == -1016
        # past the limit: the slow path, which agrees with the fast one term by term while |cx·v| < limit ...
        for th in (math.nextafter(LIMIT * math.log(2) / T, math.inf) * (1 + 1e-12), 800.0, 1e7, 1e12, 1e300):
            cx = column_entry(th, K64)
            assert outside(cx), th
            for v in (1.0, 12345.0, 2.0 ** 30, vmax):
                s = term_slow(cx, v, tabb, low_dword_k)
                old = term_present(cx, v, t64)
                ref = exact(cx, v)
                if abs(cx * v) < LIMIT:
                    assert s == term_fast(cx, v, tabb), (th, v)
                if ref > mp.mpf(2) ** -1022:
                    assert relerr(s, ref) < TOL, (th, v)
                else:                                           # ... and below the normal range gives the parent's denormal, or 0
                    assert abs(s - old) <= 2.0 ** -1074 + 8e-14 * old, (th, v, s, old)
                    if old == 0.0 and ref < mp.mpf(2) ** -1076:
                        assert s == 0.0, (th, v, s)
        # the denormal range itself, argument by argument
        for arg in np.linspace(708.0, 746.0, 39):
            cx = column_entry(float(arg), K64)
            s, old = term_slow(cx, vmax, tabb, low_dword_k), term_present(cx, vmax, t64)
            assert abs(s - old) <= 2.0 ** -1074 + 8e-14 * old, (arg, s, old)
            assert abs(mp.mpf(s) - exact(cx, vmax)) <= mp.mpf(2) ** -1074, arg
        # past 2^31 in the scaled argument (θ·Δtmax = 1e8 is 9.2e9), and rates that are not numbers
        cx = column_entry(1e8, K64)
        assert abs(cx * vmax) > 2.0 ** 31 and term_slow(cx, vmax, tabb, low_dword_k) == 0.0
        assert term_present(cx, vmax, t64) == 0.0
        for bad in (math.inf, -math.inf, math.nan):
            cx = column_entry(bad, K64)
            assert outside(cx)
            assert math.isnan(term_slow(cx, vmax, tabb, low_dword_k)) and math.isnan(term_present(cx, vmax, t64))
    return worst_new, worst_old, worst_move, moved


def test_both_paths_against_exp_and_the_present_helper(tables, terms):
    worst_new, worst_old, worst_move, moved = compare(tables, terms)
    print(f"worst relative error: new {worst_new:.3g}, present helper {worst_old:.3g}; largest move {worst_move:.3g}; "
          f"{moved} of {len(terms)} terms change bits")
    assert worst_new < TOL


def test_limit_in_the_models_terms():
    """θ·Δtmax = 700 is inside, 704 and beyond outside: 1015.625·ln 2 = 703.98."""
    assert not outside(column_entry(700.0, K64)) and not outside(column_entry(1e-6, K64))
    assert not outside(column_entry(-700.0, K64))             # (a negative rate: the same margin on the other side)
    assert outside(column_entry(704.0, K64)) and outside(column_entry(800.0, K64)) and outside(column_entry(1e7, K64))
    assert abs(LIMIT * math.log(2) / T - 703.98) < 0.01


def test_planted_bias_left_out_of_one_entry(tables, terms):
    t64, good = tables
    bad = list(good)
    bad[37] = bits(t64[37])
    with pytest.raises(AssertionError):
        compare(tables, terms, tabb=bad, extremes=False)


def test_planted_low_dword_k_on_the_slow_path(tables, terms):
    compare(tables, terms[:50], low_dword_k=True, extremes=False)     # (inside the limit the low dword IS k: nothing to see)
    with pytest.raises(AssertionError):
        compare(tables, terms[:50], low_dword_k=True, extremes=True)
