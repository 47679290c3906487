"""TEST INFRASTRUCTURE - the rounding budget of the GLS direct sums (csrc/gls.hip, gls_sums.h, gls_ragged.hip), derived
from the arithmetic and never from what the device returns, with the inputs and the exact reference that let a test
gate on it.  Plain numpy; imports nothing from ``periodicity_amd``.  DESIGN.md 4.1m carries the derivation line by line
(D1 ... D12 below name its lines); tests/test_gls_error_budget_host.py checks everything here that needs no device.

Lattice inputs.  ``t = JD + T 2^-16`` (integer ``T < 2^28``, sorted) makes ``t' = t - t[0]`` exact; ``f0 = F0 2^-22``,
``delta = D 2^-22`` make every ``f0 + j delta`` an exact double, so the device's fill rule ``fl(f0 + fl(j delta))``,
numpy's and the real number coincide, and ``f t' mod 1 = (F T' mod 2^38) / 2^38`` in integers.  What is left between the
device and the exact sums is the kernel's own arithmetic.  On a grid near 1000 cycles per day ``F T'`` needs up to 60
bits: the ``lo`` term of ``frac_product`` is live in every phase product.  (Below ~2^25 2^-22 = 8 cycles per day the
product fits 53 bits and ``lo`` is zero: the low grids test everything but that term.)

The budget.  u = 2^-53.  Every raw sum the device accumulates obeys ``|dev - exact| <= C u A`` with A the sum of the
absolute weights (sum w |y'| for Sh, Ch; sum w for S, C, SS, SC) and C = C_trig + C_sum + C_pro:

D1  sincos of a reduced phase, E_SC = 8: ``frac_product`` rounds r once (<= u/2 cycles = pi u rad), x = z * fl(2 pi)
    adds 1.1 u rad, the two Horner chains and their closing fma 2.7 u (norm of the pair); 4.25 + 2.7 < 8.
D2  one plane rotation ``rot2``, RHO = 2: a product and an fma per component, norm <= u (|y.x| |x| + |result|).
D3  lane chain, row[8 COLS + b] = step^b, b <= 7: b E_SC + (b - 1) RHO <= 7 E_SC + 6 RHO = 68.
D4  column chain, row[q] = base step8^q, q <= 8 COLS - 1: (E_SC + 1) + q (E_SC + RHO); the + 1 is the scaling by sqrt(w).
D5  seed = rot2(column entry, lane entry): D3 + D4 + RHO.
D6  ``walk_grid``, k = K - 1 steps.  The computed per-sample rotation M~ = [[c~, s~], [-s~, c~]] obeys
    M~^2 = 2 c~ M~ - (1 + eps) I with |eps| = |c~^2 + s~^2 - 1| <= 2 * 2.7 u (only the radial part of D1 changes the
    norm).  The recurrence x[k+1] = 2 c~ x[k] - x[k-1] therefore follows y[k] = M~^k seed up to local errors
    ETA = 5.4 + 1 (the fma) < 7 per step and RHO at the first rotation, which propagate through U_m(c~),
    |U_m| <= m + 1: RHO k + ETA k (k - 1) / 2.  M~^k differs from the exact rotation by k E_SC.
D7  quadratic sums (s^2, s c of the carried values): twice the linear error plus the product's rounding, 2 C + 1.
D8  C_sum: one rounding per accumulating fma along a thread's run of samples, then the adds of the SPLIT fold, of
    ``gls_finish_kernel`` (lane q takes parts q, q + 4, ...; two shuffles) - the longest chain of roundings a term passes.
D9  C_pro, the prologue: w~ = fl(fl(1 / fl(e^2)) / W~) (3 + C_W), carried as sqrt (2), times y' (1), y' = fl(y - ybar~)
    (1): 7 + C_W, with C_W the chain of W's own sum (stride loop, wave tree 6, waves).  ybar~ is off by at most
    C_YBAR u sum w |y|, C_YBAR = 2 C_W + 5, which enters Sh and Ch through S and C: an extra C_YBAR u (sum w |y|) (sum w).
    YY carries 2 C_W + 8 relative; W (the psd factor, and C2 = Wsum - 2 SS) C_W.
D10 pair kernel: no recurrence.  u+- = a c_m +- b s_m from the seed at the thread's centre (D5 with 1.5 u more cycles
    of phase rounding in the base: three reduced phases are added, + 20) and the offset table (E_SC; E_SC2 = 12 for the
    doubled angle): linear E_seed + E_SC + 2, quadratic 2 E_seed + E_SC2 + 2 E_SC + 8.  A frequency's sum is P +- Q of two
    accumulated sums (three for SS with G_m): C_sum counts its run twice (three times).
D11 shared time axis: ``sincos_cycles_half`` evaluates at a quarter of the angle (4.1 u) and doubles twice; the map
    (s, c) -> (2 s c, 1 - 2 s^2) has norm <= sqrt(4 + 16 s^2) (3.47 for |s| <= sin(pi / 4), then 4.47) and rounds
    1.5 u: E_HALF = ((4.1 * 3.47) + 1.5) * 4.47 + 1.5 < 72.  Two per lane: the second frequency is one rotation by a
    second such sincos, 2 E_HALF + RHO.  A wave's run is the whole curve; equal weights scale by 1 / W after (+ 2).
D12 raw sums: the rotation back by f t0 (E_SC and three roundings on |S| + |C|), + 16.

The power.  ``bound_p`` is first order: |dp/dsigma| by central differences of ``scan_oracle.gls_epilogue`` in long
double, times the budget of each sum, plus the YY and W terms of D9 and one epilogue term: Sw = sqrt(1/2) sqrt(1 - C2w)
cancels where the rotation angle is small, its error u / |Sw| is NOT a relative one, and p answers to it in first order,
so |dp/dSw| u / |Sw| is added (from a restatement of the epilogue that takes the perturbation).  The gate is
``|p_dev - p_exact| <= 2 bound_p + 64 u |p_exact|``: the second order is (C u)^2 ~ 1e-24; the epilogue's other ~25
roundings are each a relative u on a quantity that is a smooth function of the sums with the same partial derivatives,
i.e. a perturbation of at most u A per sum and rounding - 25 where C is never below 360 - and its last operations act on p
itself (a few u |p|).  The reference's own epilogue runs in long double but takes sqrt(0.5) from double: 2 u |p|.
"""
import numpy as np

from oracle import c_oracle as co
from oracle import scan_oracle as so

U = 2.0 ** -53
JD = 2454900.5
TBITS, FBITS = 16, 22
CAP = 1e-10          # at most 1 % of a case's bins may carry a wider bound_p
E_SC, E_SC2, RHO, ETA, E_HALF = 8, 12, 2, 7, 72


# ---- lattice inputs ----------------------------------------------------------------------------------------------------
def lattice_curve(n, seed, period, span):
    """``sinusoid()`` of tests/test_gls_dispatch_gpu.py on the time lattice: ``(t, y, dy, T)``, ``t = JD + T 2^-16``."""
    assert span <= 4096
    rng = np.random.default_rng(seed)
    T = np.sort(rng.integers(0, int(span * 2 ** TBITS), n, dtype=np.int64))
    t = JD + T / 2.0 ** TBITS
    dy = rng.uniform(0.05, 0.2, n)
    y = 1.0 + 0.5 * np.sin(2 * np.pi * t / period) + dy * rng.standard_normal(n)
    return t, y, dy, T


def lattice_step(span, oversample=5):
    """``(F0, D)``: delta = D 2^-22 ~ 1 / (oversample span), f0 = F0 2^-22 = delta / 2 (rounded down)."""
    D = int(round(2 ** FBITS / (oversample * span)))
    return D // 2, D


def high_j_begin(D, span, cycles=4e6):
    """The slab whose first bin spans ~``cycles`` cycles over the baseline."""
    return int(round(cycles / span * 2 ** FBITS / D))


def lattice_grid(F0, D, nf, j_begin=0):
    """``(frequencies, F)`` with F = F0 + (j_begin + j) D the integer numerators."""
    F = F0 + (j_begin + np.arange(nf, dtype=np.int64)) * D
    return F / 2.0 ** FBITS, F


def exact_fraction(F, Tp):
    """f t' mod 1 for f = F 2^-22, t' = Tp 2^-16 as a long double, from integers alone (F Tp < 2^63)."""
    F, Tp = np.asarray(F, dtype=np.int64), np.asarray(Tp, dtype=np.int64)
    assert int(F.max(initial=0)).bit_length() + int(Tp.max(initial=0)).bit_length() <= 63
    m = (F * Tp) & ((1 << (TBITS + FBITS)) - 1)
    return m.astype(np.longdouble) / np.longdouble(2 ** (TBITS + FBITS))


# ---- the exact reference -----------------------------------------------------------------------------------------------
def prologue_ld(y, dy, fit_mean):
    """spectral.py:99-108, 120 in long double: ``(w, y', YY, err)`` with sum w = 1."""
    y = np.asarray(y, dtype=np.longdouble)
    err = np.ones_like(y) if dy is None else np.asarray(dy, dtype=np.longdouble)
    w = 1 / (err * err)
    w = w / w.sum()
    yc = y - np.dot(w, y) if fit_mean else y
    return w, yc, np.dot(w, yc * yc), err


def epilogue_ld(Sh, Ch, S2, C2, S, C, YY, fit_mean, psd, err, dSw=0):
    """``scan_oracle.gls_epilogue`` restated so that Sw can be perturbed (``dSw``); equal to it at dSw = 0 (host test)."""
    tan2 = (S2 - 2 * S * C) / (C2 - (C * C - S * S)) if fit_mean else S2 / C2
    norm = np.sqrt(1 + tan2 * tan2)
    S2w, C2w = tan2 / norm, 1 / norm
    Cw = np.sqrt(0.5) * np.sqrt(1 + C2w)
    Sw0 = np.sqrt(0.5) * np.sign(S2w) * np.sqrt(1 - C2w)
    Sw = Sw0 + dSw
    YC, YS = Ch * Cw + Sh * Sw, Sh * Cw - Ch * Sw
    CC = 0.5 * (1 + C2 * C2w + S2 * S2w)
    SS = 0.5 * (1 - C2 * C2w - S2 * S2w)
    if fit_mean:
        CC = CC - (C * Cw + S * Sw) ** 2
        SS = SS - (S * Cw - C * Sw) ** 2
    power = YC * YC / CC + YS * YS / SS
    power = power * (0.5 * (err ** -2.0).sum()) if psd else power / YY
    return power, Sw0


def exact_sums(t, y, dy, freq, fit_mean):
    """``(sums [nf][6] long double, w, y', YY, err)`` by ``oracle_gls_sums_reduced`` on the long-double prologue."""
    w, yc, YY, err = prologue_ld(y, dy, fit_mean)
    return co.gls_sums_reduced(t, w * yc, w, freq), w, yc, YY, err


def power_of(sums, YY, err, fit_mean, psd):
    Sh, Ch, S, C, S2, C2 = (sums[:, q] for q in range(6))
    return so.gls_epilogue(Sh, Ch, S2, C2, S if fit_mean else None, C if fit_mean else None, YY, fit_mean, psd, err)


# ---- the constants -----------------------------------------------------------------------------------------------------
def c_weight_sum(n, block, wide=False):
    """D9: the chain of roundings of W = sum err^-2 (and of every prologue sum taken the same way)."""
    if wide:   # gls_prep_wide_a / _b / _c: <= 512 workgroups of 256, then the partials folded by 256 threads
        nparts = min(512, -(-n // 1024))
        return -(-n // (nparts * 256)) + 6 + 4 + -(-nparts // 256) + 6 + 4
    return -(-n // block) + 6 + block // 64


def c_trig(K, cols, pair=False):
    """D3 - D6 (D10 for the pair kernel): the error of a carried {sin, cos} pair, in u of its scale."""
    lane = 7 * E_SC + 6 * RHO
    column = (E_SC + 1) + (8 * cols - 1) * (E_SC + RHO)
    seed = lane + column + RHO
    if pair:
        return seed + 20 + E_SC + 2
    k = K - 1
    return seed + k * E_SC + RHO * k + ETA * k * (k - 1) // 2


def route_constants(rec, n, pair=False, raw=False):
    """``(C_lin, C_quad, C_W, C_YBAR, C_YY)`` of one launch, from the dispatch record of the hook (``route``, ``K``,
    ``S``, ``parts``, ``z_len``, ``bal_slots``, ``wide_prep``; ``route = "ragged"`` for gls_ragged.hip) and the curve's
    length."""
    route = rec["route"]
    if route in ("shared", "shared2"):
        cw = c_weight_sum(n, 1024)
        lin = E_HALF if route == "shared" else 2 * E_HALF + RHO
        csum = n + 1 + 2
        pro = 7 + cw
        return lin + csum + pro, 2 * lin + 1 + csum + pro, cw, 2 * cw + 5, 2 * cw + 8
    if route == "ragged":
        K, S, cols, chunk, cw = 8, 1, 2, 64, c_weight_sum(n, 256)
        stretch, after = n, 0
    else:
        K, S = rec["K"], rec["S"]
        cols, chunk = 256 // S // 64, 64 if S == 1 else 128
        cw = c_weight_sum(n, 1024, wide=bool(rec.get("wide_prep")))
        stretch, after = n, 0
        if route == "parts":
            stretch, after = rec["z_len"], -(-rec["parts"] // 4) + 2
        elif route == "balanced":
            after = 1 + 2      # a tile falls into at most three runs
    run = -(-stretch // chunk) * (chunk // S)      # D8: a wave takes 1 / S of every chunk
    csum = run + (S - 1) + after
    pro = 0 if raw else 7 + cw
    trig = c_trig(K, cols, pair)
    if pair:
        quad = 2 * (trig - E_SC - 2) + E_SC2 + 2 * E_SC + 8
        return trig + 2 * csum + pro, quad + 3 * csum + pro, cw, 2 * cw + 5, 2 * cw + 8
    if raw:
        return trig + csum + 16, 0, 0, 0, 0
    return trig + csum + pro, 2 * trig + 1 + csum + pro, cw, 2 * cw + 5, 2 * cw + 8


# ---- the per-bin bound on the power ------------------------------------------------------------------------------------
def bound_power(sums, w, y, yc, YY, err, fit_mean, psd, consts):
    """First-order bound on |p_dev - p_exact| per bin (long double) from the budgets of the sums; see the module
    docstring.  ``y``: the values before centring (for D9's ybar term)."""
    c_lin, c_quad, c_w, c_ybar, c_yy = consts
    u = np.longdouble(U)
    A_w, A_y = w.sum(), np.dot(w, np.abs(yc))
    ybar_term = c_ybar * u * np.dot(w, np.abs(np.asarray(y, dtype=np.longdouble))) * A_w if fit_mean else 0
    d_lin_y = c_lin * u * A_y + ybar_term
    d_lin_w = c_lin * u * A_w
    d_quad = c_quad * u * A_w
    # the device's SS, SC reach the epilogue as C2 = Wsum - 2 SS, S2 = 2 SC
    budget = [d_lin_y, d_lin_y, d_lin_w, d_lin_w, 2 * d_quad, 2 * d_quad + c_w * u * A_w]
    scale = [A_y, A_y, A_w, A_w, A_w, A_w]

    def p_at(v, yy=YY, dSw=0):
        return epilogue_ld(v[:, 0], v[:, 1], v[:, 4], v[:, 5], v[:, 2], v[:, 3], yy, fit_mean, psd, err, dSw)[0]

    def p_ref(v, yy=YY):
        return power_of(v, yy, err, fit_mean, psd)

    bound = np.zeros(sums.shape[0], dtype=np.longdouble)
    for q in range(6):
        if q in (2, 3) and not fit_mean:
            continue
        h = np.longdouble(1e-7) * scale[q]
        hi, lo = sums.copy(), sums.copy()
        hi[:, q] += h
        lo[:, q] -= h
        bound += np.abs(p_ref(hi) - p_ref(lo)) / (2 * h) * budget[q]
    p = p_ref(sums)
    if psd:
        bound += np.abs(p) * c_w * u                      # the factor W / 2
    else:
        bound += np.abs(p) * c_yy * u                     # p = (...) / YY
    Sw = epilogue_ld(sums[:, 0], sums[:, 1], sums[:, 4], sums[:, 5], sums[:, 2], sums[:, 3], YY, fit_mean, psd, err)[1]
    h = np.longdouble(1e-7)
    bound += np.abs(p_at(sums, dSw=h) - p_at(sums, dSw=-h)) / (2 * h) * u / np.maximum(np.abs(Sw), u)
    return bound


def gate(bound, p_exact):
    return 2 * bound + 64 * np.longdouble(U) * np.abs(p_exact)


# ---- which bins the oracle is asked for --------------------------------------------------------------------------------
def pick_bins(nf, tile, seams=(), extra=(), limit=1024, seed=1):
    """Stratified: first and last bin of every tile (of as many tiles, evenly spread, as half the limit holds), the
    bins round every seam, ``extra`` (the expected peak and its neighbours), then random ones up to ``limit``."""
    rng = np.random.default_rng(seed)
    starts = np.arange(0, nf, tile, dtype=np.int64)
    if 2 * starts.size > limit // 2:
        starts = starts[np.unique(np.linspace(0, starts.size - 1, limit // 4).astype(np.int64))]
    ends = np.minimum(starts + tile, nf) - 1
    near = [np.arange(s - 1, s + 2) for s in seams] + [np.asarray(extra, dtype=np.int64)]
    fixed = np.unique(np.concatenate([starts, ends, [0, nf - 1]] + near).astype(np.int64))
    fixed = fixed[(fixed >= 0) & (fixed < nf)]
    room = max(0, limit - fixed.size)
    pick = np.unique(np.concatenate([fixed, rng.integers(0, nf, room)]))
    assert pick.size <= limit
    return pick


# ---- the cases: shared by the host test (properties of the inputs, the 1 % cap) and the GPU test -----------------------
# A group is one child interpreter (the PDC_GLS_* switches are read once per process): its switches, what the dispatch
# hook must report for every case of it (``tiles`` and the like are filled in per case), whether the mirrored-pair
# kernel must have run, and its cases.  Every group runs fit_mean on and off, psd once, and one case on the slab at
# ~4e6 cycles ("high").
def _curve_case(name, n, nf, fit_mean, psd, high, seed, span, period=37.3):
    F0, D = lattice_step(span)
    return dict(name=name, kind="scan", n=n, nf=nf, fit_mean=fit_mean, psd=psd, seed=seed, span=span, period=period,
                F0=F0, D=D, j_begin=high_j_begin(D, span) if high else 0, B=1, shared_t=False)


def _trio(n, nf, seed, span):
    return [_curve_case("mean", n, nf, True, False, False, seed, span),
            _curve_case("psd", n, nf, False, True, False, seed + 1, span),
            _curve_case("high", n, nf, True, False, True, seed + 2, span)]


def _general(K, S, pair=0, lead=0):
    tile = 256 // S * K
    return dict(env=dict(PDC_GLS_K=K, PDC_GLS_S=S, PDC_GLS_BAL=0, PDC_GLS_PAIR=pair, PDC_GLS_LEAD=lead), pair=bool(pair),
                want=dict(route="general", K=K, S=S, parts=1, wide_prep=0, bal_slots=0, tiles=-(-4099 // tile),
                          lead_swap=int(bool(lead and pair and S <= 2))),
                cases=_trio(1031, 4099, 100 * K + S, 1031))


def _shared_cases():
    F0, D = 47395, 8808            # f0 = 0.0113, delta = 0.0021, as the dispatch tests' shared grids
    out = []
    for name, fit_mean, psd, high in (("mean", True, False, False), ("psd", False, True, False), ("high", True, False, True)):
        out.append(dict(name=name, kind="scan", n=257, nf=193, fit_mean=fit_mean, psd=psd, seed=500 + len(out), span=40,
                        period=3.3, F0=F0, D=D, j_begin=high_j_begin(D, 40) if high else 0, B=129, shared_t=True))
    return out


def _shared(kernel):
    with_dy, extra = {"two_per_lane": (True, {}), "one_per_lane": (True, {"PDC_GLS_SH2": 0}),
                      "equal_weights": (False, {})}[kernel]
    per_group = {"two_per_lane": 64, "one_per_lane": 128, "equal_weights": 256}[kernel]
    pad, per_lane = (256, 1) if kernel == "equal_weights" else (128, 2 if kernel == "two_per_lane" else 1)
    bpad = -(-129 // pad) * pad
    cases = _shared_cases()
    if kernel == "two_per_lane":
        cases.append(dict(name="boot", kind="boot", n=257, nf=193, fit_mean=True, psd=False, seed=77, span=40, period=3.3,
                          F0=47395, D=8808, j_begin=0, B=130, shared_t=True))
    return dict(env=dict(PDC_GLS_SHARED=1, **extra), pair=False, with_dy=with_dy,
                want=dict(route="shared2" if per_lane == 2 else "shared", K=per_lane, S=0, bpad=bpad,
                          groups=bpad // per_group, tiles=-(-193 // (64 * per_lane)), parts=1, wide_prep=0),
                cases=cases)


def _ragged_cases():
    out = []
    for name, fit_mean, psd, high in (("mean", True, False, False), ("nomean", False, False, False),
                                      ("psd", True, True, False), ("high", True, False, True)):
        F0, D = lattice_step(200)
        jb = high_j_begin(D, 200) if high else 0
        out.append(dict(name=name, kind="ragged", ns=[191, 192, 193], nfs=[1025, 700, 1024], fit_mean=fit_mean, psd=psd,
                        seed=900 + len(out), span=200, period=7.3, F0s=[F0 + jb * D, F0 + jb * D + 1, F0 + jb * D + 2],
                        Ds=[D, D + 1, D - 1]))
    return out


# (The routes that need >= 16384 samples run S = 4: a wave's run of a part is a quarter of it, so that C_sum does not
# drown C_trig - with S = 1 their budgets could not see a sincos polynomial one term short)
GROUPS = {}
for _K in (4, 8, 16):
    for _S in (1, 2, 4):
        GROUPS[f"general_k{_K}_s{_S}"] = _general(_K, _S)
GROUPS.update({
    "pair_s1_lead": _general(16, 1, pair=1, lead=1),
    "pair_s2": _general(16, 2, pair=1),
    "pair_s2_lead": _general(16, 2, pair=1, lead=1),
    "pair_s4": _general(16, 4, pair=1),
    "parts_grid_y": dict(env=dict(PDC_GLS_Z=2, PDC_GLS_K=8, PDC_GLS_S=4), pair=False, limit=256,
                         want=dict(route="parts", K=8, S=4, parts=2, parts_by_xcd=0, z_len=8320, wide_prep=1, tiles=2,
                                   bal_slots=0),
                         cases=_trio(16400, 700, 31, 4000)),
    "parts_by_xcd": dict(env=dict(PDC_GLS_Z=9, PDC_GLS_K=8, PDC_GLS_S=2), pair=False, limit=256,
                         want=dict(route="parts", K=8, S=2, parts=9, parts_by_xcd=1, z_len=2176, wide_prep=1, tiles=1,
                                   bal_slots=0),
                         cases=_trio(18500, 700, 41, 4000)),
    "wide_prologue": dict(env=dict(PDC_GLS_Z=1, PDC_GLS_K=8, PDC_GLS_S=4, PDC_GLS_BAL=0), pair=False, limit=256,
                          want=dict(route="general", K=8, S=4, parts=1, wide_prep=1, tiles=2, bal_slots=0),
                          cases=_trio(16385, 700, 51, 4000)),
    "balanced_forced_pair": dict(env=dict(PDC_GLS_K=16, PDC_GLS_S=4, PDC_GLS_BAL=1), pair=True,
                                 want=dict(route="balanced", K=16, S=4, parts=1, parts_by_xcd=0, tiles=257, bal_slots=512,
                                           bal_chunks=32, wide_prep=0),
                                 cases=[_curve_case("mean", 3969, 257 * 1024 - 5, True, False, False, 61, 3969),
                                        _curve_case("high", 3969, 257 * 1024 - 5, True, False, True, 62, 3969)]),
    "balanced_forced_plain": dict(env=dict(PDC_GLS_K=16, PDC_GLS_S=2, PDC_GLS_BAL=1, PDC_GLS_PAIR=0), pair=False,
                                  want=dict(route="balanced", K=16, S=2, parts=1, parts_by_xcd=0, tiles=301, bal_slots=512,
                                            bal_chunks=40, wide_prep=0),
                                  cases=[_curve_case("psd", 5000, 300 * 2048 + 1000, False, True, False, 63, 4000)]),
    "balanced_by_the_model": dict(env={}, pair=True,
                                  want=dict(route="balanced", K=16, S=4, parts=1, parts_by_xcd=0, tiles=385, bal_slots=512,
                                            bal_chunks=32, wide_prep=0),
                                  cases=[_curve_case("mean", 4001, 385 * 1024 - 3, True, False, False, 64, 4001)]),
    "shared_two_per_lane": _shared("two_per_lane"),
    "shared_one_per_lane": _shared("one_per_lane"),
    "shared_equal_weights": _shared("equal_weights"),
    "ragged": dict(env={}, pair=False, want=dict(route="ragged"), cases=_ragged_cases()),
})
SHARED_CURVES = [0, 63, 64, 127, 128]      # the curves the oracle checks: both sides of every curve-group boundary
BOOT_REPLICATES = [0, 64, 129]


def case_arrays(group, case):
    """The input arrays of one case (lattice times, ordinary noisy-sinusoid values)."""
    with_dy = GROUPS[group].get("with_dy", True)
    if case["kind"] == "ragged":
        parts = [lattice_curve(n, case["seed"] + 10 * b, case["period"], case["span"]) for b, n in enumerate(case["ns"])]
        return dict(t=np.concatenate([p[0] for p in parts]), y=np.concatenate([p[1] for p in parts]),
                    dy=np.concatenate([p[2] for p in parts]), T=np.concatenate([p[3] for p in parts]))
    t, y, dy, T = lattice_curve(case["n"], case["seed"], case["period"], case["span"])
    out = dict(t=t, T=T)
    if case["kind"] == "boot":
        out.update(y=y, picks=np.random.default_rng(9).integers(0, case["n"], (case["B"], case["n"])).astype(np.int32))
        if with_dy:
            out["dy"] = dy
        return out
    if case["B"] > 1:
        rng = np.random.default_rng(case["seed"] + 1000)
        out["y"] = (1.0 + np.sin(2 * np.pi * t / case["period"])[None, :] + 0.5 * rng.standard_normal((case["B"], case["n"]))).ravel()
        if with_dy:
            out["dy"] = rng.uniform(0.1, 0.5, (case["B"], case["n"])).ravel()
        return out
    out.update(y=y, dy=dy)
    return out


def case_curves(group, case, arrays):
    """``[(label, t, y, dy, F0, D, j_begin, nf, row, bin offset)]``: the single curves of a case the oracle is asked for;
    ``row`` finds a curve's peak and, with ``offset`` (ragged: into the flat spectrum), its spectrum in what the device
    returns."""
    if case["kind"] == "ragged":
        out, lo, fo = [], 0, 0
        for b, (n, nf) in enumerate(zip(case["ns"], case["nfs"])):
            s = slice(lo, lo + n)
            out.append((f"curve {b}", arrays["t"][s], arrays["y"][s], arrays["dy"][s], case["F0s"][b], case["Ds"][b], 0, nf,
                        b, fo))
            lo, fo = lo + n, fo + nf
        return out
    t, n, nf = arrays["t"], case["n"], case["nf"]
    dy = arrays.get("dy")
    if case["kind"] == "boot":
        pk = arrays["picks"]
        return [(f"replicate {b}", t, arrays["y"][pk[b]], None if dy is None else dy[pk[b]], case["F0"], case["D"], 0, nf,
                 b, 0) for b in BOOT_REPLICATES]
    if case["B"] > 1:
        y = arrays["y"].reshape(case["B"], n)
        dy = None if dy is None else dy.reshape(case["B"], n)
        return [(f"curve {b}", t, y[b], None if dy is None else dy[b], case["F0"], case["D"], case["j_begin"], nf, b, 0)
                for b in SHARED_CURVES]
    return [("curve", t, arrays["y"], dy, case["F0"], case["D"], case["j_begin"], nf, 0, 0)]


def case_tile(group, case):
    """Frequencies per tile of the kernel the group's record names."""
    want = GROUPS[group]["want"]
    if want["route"] == "ragged":
        return 1024
    if want["route"] in ("shared", "shared2"):
        return 64 * want["K"]
    return 256 // want["S"] * want["K"]


def case_picks(group, case, nf, j_begin, F0, D, extra=()):
    """The bins of one curve the oracle is asked for: ``pick_bins`` with the expected peak (1 / period) and two bins
    either side of it, at most 1024 bins per case."""
    curves = 3 if case["kind"] in ("ragged", "boot") else (len(SHARED_CURVES) if case.get("B", 1) > 1 else 1)
    limit = GROUPS[group].get("limit", 1024) // curves
    peak = int(round((2 ** FBITS / case["period"] - F0) / D)) - j_begin
    near = [j for j in range(peak - 2, peak + 3) if 0 <= j < nf] + [int(j) for j in extra if 0 <= j < nf]
    if nf <= limit:
        return np.arange(nf, dtype=np.int64)
    return pick_bins(nf, case_tile(group, case), extra=near, limit=limit)


def curve_reference(group, case, curve, consts, extra=()):
    """``(pick, p_exact, bound, unit)`` of one curve of a case: the oracle's power on the picked bins, ``bound_power``, and
    the unit the 1e-10 cap is counted in: 1 for the normalised power (<= 1), W YY / 2 with psd, which is the normalised
    power times exactly that."""
    label, t, y, dy, F0, D, j_begin, nf, row, offset = curve
    pick = case_picks(group, case, nf, j_begin, F0, D, extra)
    freq = lattice_grid(F0, D, nf, j_begin)[0][pick]
    sums, w, yc, YY, err = exact_sums(t, y, dy, freq, case["fit_mean"])
    p = power_of(sums, YY, err, case["fit_mean"], case["psd"])
    unit = 0.5 * (err ** -2.0).sum() * YY if case["psd"] else np.longdouble(1)
    return pick, p, bound_power(sums, w, y, yc, YY, err, case["fit_mean"], case["psd"], consts), unit


def expected_record(group, case):
    """What the hook must report for this case (the group's ``want``); the record ``route_constants`` takes where no
    device is at hand."""
    return dict(GROUPS[group]["want"])


# ---- the raw sums (pdc_trig_sums, MODE_RAW): n in {129, 4000}, 2049 bins, from delta / 2 and from ~4e6 cycles ----------
RAW = {}
for _n in (129, 4000):
    for _high in (False, True):
        _F0, _D = lattice_step(_n if _n > 129 else 129)
        RAW[f"n{_n}_{'high' if _high else 'low'}"] = dict(n=_n, nf=2049, span=max(_n, 129), seed=7 + _n + _high,
                                                        F0=_F0 + (high_j_begin(_D, max(_n, 129)) * _D if _high else 0), D=_D)


def raw_inputs(case):
    t, y, dy, T = lattice_curve(case["n"], case["seed"], 37.3, case["span"])
    h = (y - y.mean()) / dy ** 2      # signed weights of ordinary size
    return t, h, T


def raw_exact(case, pick):
    """S, C of ``sum h sin / cos(2 pi f t)`` over the ABSOLUTE times, in long double: the reduced sums over t', turned by
    f t[0] mod 1 from integers."""
    t, h, T = raw_inputs(case)
    freq, F = lattice_grid(case["F0"], case["D"], case["nf"])
    hl = np.asarray(h, dtype=np.longdouble)
    sums = co.gls_sums_reduced(t, hl, hl, freq[pick])
    T0 = int(JD * 2 ** TBITS) + int(T[0])
    frac = np.array([np.longdouble((int(f) * T0) % (1 << (TBITS + FBITS))) for f in F[pick]], dtype=np.longdouble)
    ang = so.TWO_PI_L * frac / np.longdouble(2 ** (TBITS + FBITS))
    s0, c0 = np.sin(ang), np.cos(ang)
    return sums[:, 0] * c0 + sums[:, 1] * s0, sums[:, 1] * c0 - sums[:, 0] * s0, np.abs(hl).sum()
