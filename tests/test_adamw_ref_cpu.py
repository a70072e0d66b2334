"""tests/adamw_ref.py qualified without a GPU: the exact designs give their closed-form bits under every contraction, the
float32 restatement stays within half the bar of the float64 reference, every planted error is caught, and step_advance's
restatement is admitted by its bar.

The half-bar margin.  `step32` in its three contraction variants must stay within HALF of `bar` against `step64`; the
other half is the margin for what the device may do differently from numpy: its choice of which multiply-adds to fuse, and
its sqrtf and fp32 division.  That margin rests on the build flags of csrc/Makefile: `-O3 -ffp-contract=fast` and nothing
that loosens fp32 arithmetic (no -ffast-math, no -fgpu-flush-denormals-to-zero, and
-fhip-fp32-correctly-rounded-divide-sqrt left at its default, on), so that sqrtf and `/` round correctly and subnormals
are kept.  test_build_flags_behind_the_margin pins the flags that can be read from the Makefile."""
import os
import re

import numpy as np
import pytest
import torch

import adamw_ref as R
from test_model_ema_gpu import _launcher_constants, _sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = (False, True, "right")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_build_flags_behind_the_margin():
    mk = open(os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd", "csrc", "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1)
    print("CXXFLAGS", flags)
    assert "-ffp-contract=fast" in flags
    for loose in ("-ffast-math", "-Ofast", "-funsafe-math", "-fgpu-flush-denormals-to-zero", "-fno-hip-fp32-correctly-rounded-divide-sqrt",
                  "-fapprox-func", "-freciprocal-math"):
        assert loose not in mk, loose


def test_what_each_size_exercises():
    """_sizes() (imported, not copied) walked as the kernels walk: tail alone; one remainder group; exact paired trips; two
    workgroups with paired and remainder lanes and a tail; the capped grid with three trips, one remainder lane, a tail."""
    threads, cap = _launcher_constants()
    s = _sizes()
    got = [R.walk(n, threads, cap) for n in s]
    for n, g in zip(s, got):
        print(n, g)
    assert len(s) == 7
    for g in got[:2]:                                                     # 1, 3
        assert g["max_groups"] == 0 and g["tail"] in (1, 3) and g["grid"] == 1
    assert got[2] == dict(grid=1, tail=0, trips0=0, rem_lanes=1, max_groups=1)                 # 4
    assert got[3] == dict(grid=1, tail=3, trips0=0, rem_lanes=1, max_groups=1)                 # 7
    assert got[4] == dict(grid=1, tail=0, trips0=1, rem_lanes=0, max_groups=2)                 # THREADS * 8
    g = got[5]                                                                                 # 2451
    assert g["grid"] == 2 and g["tail"] == 3 and g["trips0"] == 1 and 0 < g["rem_lanes"] < 2 * threads
    assert got[6] == dict(grid=cap, tail=1, trips0=3, rem_lanes=1, max_groups=7)               # the capped grid


def test_bf16_rounding_is_torchs():
    r = np.random.default_rng(3)
    x = np.concatenate([r.standard_normal(4096).astype(np.float32) * 10.0 ** r.integers(-30, 30, 4096).astype(np.float32),
                        np.array([0.0, -0.0, np.inf, -np.inf, 1.00390625, 1.01171875, 3.3e38, 3.4e38, 1e-40], dtype=np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_bits(x), want)
    assert np.isnan(R.bf16_round(np.array([np.nan], dtype=np.float32)))[0]


# ---- exact designs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", _sizes())
@pytest.mark.parametrize("name", R.DESIGNS)
def test_exact_designs_give_their_closed_form_bits(name, n):
    d = R.design(name, n)
    kw = R.design_step_kwargs(d)
    want = d["want"]
    w64, m64, v64, _ = R.step64(d["w"], d["m"], d["v"], d["g"], **kw)
    for k, x in (("w", w64), ("m", m64), ("v", v64)):
        assert np.array_equal(x, want[k].astype(np.float64)), (k, "float64")
    for c in VARIANTS:
        got = dict(zip("wmv", R.step32(d["w"], d["m"], d["v"], d["g"], contract=c, **kw)))
        for k in "wmv":
            diff = int((_bits(got[k]) != _bits(want[k])).sum())
            assert diff == 0, (name, n, c, k, diff)
        for ce in (False, True):
            assert np.array_equal(_bits(R.ema32(np.zeros(n, np.float32), got["w"], 0.5, ce)), _bits(want["ema"])), (name, n, c, ce)
    assert bool((d["g"] != 0).all())
    if name == "first":
        assert int((want["w"] == 0).sum()) < n or n < 4
        assert want["w"][0] == -0.125 * np.sign(d["g"][0]) and d["w"][0] == 0
        if n >= 64:
            b = _bits(want["w"][d["ties"]])
            assert len(d["ties"]) == 18 and bool(((b & 0xFFFF) == 0x8000).all()), "planted w' must be bf16 ties"
            up = (R.bf16_bits(want["w"][d["ties"]]).astype(np.uint32) << 16) > (b & 0xFFFF0000)
            print("ties rounding away from zero", int(up.sum()), "towards zero", int((~up).sum()))
            assert up.any() and (~up).any()
            assert (want["w"][d["ties"]] > 0).any() and (want["w"][d["ties"]] < 0).any()


def test_a_misplaced_element_changes_an_exact_design():
    """The designs tell neighbours apart: swapping two adjacent elements, or two groups of four a grid stride apart, of any
    output changes it (so a kernel that did would be seen)."""
    threads, cap = _launcher_constants()
    for name in R.DESIGNS:
        d = R.design(name, 2451)
        for k in ("w", "m", "v"):
            x = d["want"][k]
            same_next = float((x[1:] == x[:-1]).mean())
            same_stride = float((x[4 * threads:] == x[:-4 * threads]).mean())
            print(name, k, "equal to the next element", same_next, "to the one a workgroup on", same_stride)
            assert same_next < 0.2 and same_stride < 0.2


# ---- the bar against the restatement ------------------------------------------------------------------------------------------
def _cpu_case(case, n, seed):
    """One step of a case from random state.  -> (w, m, v, g, step32 kwargs, step64 kwargs, bar kwargs, bc of t - 1)"""
    t, clip, gs, wd, lr, dev = case
    w, m, v = R.random_state(n, seed)
    g = R.random_grad(n, seed + 1, clip)
    sumsq = float(np.float32((g.astype(np.float64) ** 2).sum())) if clip else None
    bc32 = R.kernel_bc32(R.BETA1, R.BETA2, t)
    state = (np.float32(lr), *bc32) if dev else None                       # what step_advance's restatement would hold
    kw64, barkw = R.case_kwargs(case, t, sumsq, state)
    kw32 = dict(kw64, bc1=bc32[0], rbc2=bc32[1])
    prev = R.kernel_bc32(R.BETA1, R.BETA2, t - 1) if t > 1 else None
    return w, m, v, g, kw32, kw64, barkw, prev


def _ratios(got, ref, bars):
    return [R.worst_ratio(a, b, c) for a, b, c in zip(got, ref, bars)]


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_restatement_within_half_the_bar_on_the_random_cases(case):
    worst = 0.0
    for n in (7, 2451):
        w, m, v, g, kw32, kw64, barkw, _ = _cpu_case(case, n, 100 + n)
        w64, m64, v64, terms = R.step64(w, m, v, g, **kw64)
        bars = R.bar(terms, **barkw)
        for c in VARIANTS:
            r = _ratios(R.step32(w, m, v, g, contract=c, **kw32), (w64, m64, v64), bars)
            print(f"FIGURE cpu half-bar {R.CASE_IDS[R.CASES.index(case)]} n={n} contract={c}: w={r[0]:.3f} m={r[1]:.3f} v={r[2]:.3f}")
            worst = max(worst, *r)
    print("worst ratio", worst)
    assert worst <= 0.5


def _edge_run():
    w, m, v, g, where = R.edge_vector()
    lr, bc1, rbc2 = R.edge_state32()
    kw = dict(R.EDGE_HYPER, bc1=bc1, rbc2=rbc2)
    kw["lr"] = lr
    outs = [R.step32(w, m, v, g, contract=c, **kw) for c in VARIANTS]
    with np.errstate(all="ignore"):
        ref = R.step64(w, m, v, g, **kw)
        bars = R.bar(ref[3], clip=False)
    return w, m, v, g, where, outs, ref, bars


def test_edge_elements_in_the_restatement():
    """What the edge elements must do, in float32: g = 0 with v = 0 leaves m = v = 0 and moves w by the decay alone (-0.0
    stays -0.0); g = +-3e38 makes v = inf and the update 0, so w is the decayed w; a gradient whose square underflows leaves
    v = 0.  On these elements the three contraction variants agree bit for bit; wherever variants disagree anywhere in the
    vector, each stays within half the bar."""
    w, m, v, g, where, outs, ref, bars = _edge_run()
    decay = np.float32(1.0) - np.float32(R.EDGE_HYPER["lr"]) * np.float32(R.EDGE_HYPER["weight_decay"])
    w2, m2, v2 = outs[0]
    for p in where["g0_v0"] + where["g0_v0_negzero_w"]:
        assert m2[p] == 0 and v2[p] == 0 and _bits(w2[p]) == _bits(np.float32(w[p] * decay))
    assert all(_bits(w2[p]) == 0x80000000 for p in where["g0_v0_negzero_w"])
    for p in where["g_+3e38"] + where["g_-3e38"]:
        assert np.isinf(v2[p]) and np.isfinite(m2[p]) and _bits(w2[p]) == _bits(np.float32(w[p] * decay))
    for p in where["g_square_underflows"]:
        assert v2[p] == 0 and m2[p] != 0 and np.isfinite(w2[p])
    for p in where["g_square_subnormal"] + where["subnormal_v"] + where["min_subnormal_v"]:
        assert 0 < v2[p] < 1.1754944e-38, (p, v2[p])
    agree = np.ones(w.size, dtype=bool)
    lr, bc1, rbc2 = R.edge_state32()
    for c in R.all_contractions():                       # the GPU test's criterion: every combination of choices agrees
        for a, b in zip(R.step32(w, m, v, g, contract=c, **dict(R.EDGE_HYPER, lr=lr, bc1=bc1, rbc2=rbc2)), outs[0]):
            agree &= _bits(a) == _bits(b)
    special = sorted(p for k in ("g0_v0", "g0_v0_negzero_w", "g_+3e38", "g_-3e38") for p in where[k])
    print("elements on which the variants agree", int(agree.sum()), "of", w.size)
    assert agree[special].all()
    combos = R.all_contractions()
    assert len(combos) == 216 and all(R.contraction(c) in combos for c in VARIANTS)
    worst = 0.0
    assert (~agree).any()
    for combo in combos:
        o = R.step32(w, m, v, g, contract=combo, **dict(R.EDGE_HYPER, lr=lr, bc1=bc1, rbc2=rbc2))
        for a, b, c in zip(o, ref[:3], bars):
            worst = max(worst, R.worst_ratio(a[~agree], b[~agree], c[~agree]))
    print(f"FIGURE cpu half-bar edge vector, elements where the variants differ: {worst:.3f}")
    assert worst <= 0.5


# ---- planted errors -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_planted_error_is_caught(mutant):
    """Each deliberate error in step32 exceeds the bar by at least 4x on one of the random cases, or changes the bits of an
    exact design."""
    worst, where = 0.0, None
    for case, cid in zip(R.CASES, R.CASE_IDS):
        w, m, v, g, kw32, kw64, barkw, prev = _cpu_case(case, 2451, 300)
        if mutant == "bc_prev_step" and prev is None:
            continue
        w64, m64, v64, terms = R.step64(w, m, v, g, **kw64)
        r = max(_ratios(R.step32(w, m, v, g, mutant=mutant, bc_prev=prev, **kw32), (w64, m64, v64), R.bar(terms, **barkw)))
        if r > worst:
            worst, where = r, cid
    changed = 0
    for name in R.DESIGNS:
        d = R.design(name, 2451)
        got = R.step32(d["w"], d["m"], d["v"], d["g"], mutant=mutant, bc_prev=(1.0, 1.0), **R.design_step_kwargs(d))
        changed += sum(int((_bits(a) != _bits(d["want"][k])).sum()) for a, k in zip(got, "wmv"))
    print(f"{mutant}: worst |err| / bar {worst:.3g} on {where}; exact-design elements changed {changed}")
    assert worst >= 4.0 or changed > 0
    if mutant in ("decay_after", "decay_on_update"):
        assert worst >= 4.0 and "lr0.1" in where          # the order of decay and update is visible on that case


# ---- step_advance -------------------------------------------------------------------------------------------------------------
def test_step_advance_restated():
    assert int(R.mix32(np.uint32(0))) == 0 and int(R.mix32(np.uint32(1))) == 0x514E28B7      # murmur3's finaliser
    seen = set()
    for before in list(range(5)) + [999]:
        step, off, bc1, rbc2 = R.advance_ref(before, R.BETA1, R.BETA2, 4242)
        assert step == before + 1 and 0 <= off < 2 ** 32
        seen.add(off)
        b1, b2 = R.advance_bar(R.BETA1, R.BETA2, step)
        g1, g2 = R.advance32(R.BETA1, R.BETA2, step)
        r1, r2 = abs(float(g1) - bc1) / b1, abs(float(g2) - rbc2) / b2
        print(f"step {step}: offset {off:#010x} bc1 {bc1:.9g} rbc2 {rbc2:.9g}; numpy float32 |err| / bar {r1:.4f} {r2:.4f}; "
              f"powf ulps {R.powf_ulps(g1, R.BETA1, step):.3f}")
        assert r1 <= 1.0 and r2 <= 1.0
        assert abs(bc1 - (1 - 0.9 ** step)) < 1e-6 and abs(rbc2 - (1 - 0.999 ** step) ** -0.5) < 1e-3 * rbc2
    assert len(seen) == 6
