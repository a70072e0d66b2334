"""The fused clip + AdamW kernels (adamw_kernel<NT>, adamw_ema_kernel<NT>, step_advance_kernel of csrc/optim.hip) against
tests/adamw_ref.py: exact answers bit for bit at every path of the walk over the elements, the float64 reference within the
derived bar over consecutive steps, edge elements, the device step state, non-finite gradients, and the three template
instances no other test runs.  The reference, the designs and the bar are described in adamw_ref's docstring and
qualified without a GPU by tests/test_adamw_ref_cpu.py.

Every test prints FIGURE lines (worst |err| / bar per output, or the number of differing elements) before asserting."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import adamw_ref as R
from guarded import assert_guards_intact, guarded_inout, guarded_input
from test_model_ema_gpu import _sizes

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
PKG = os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd")
SIZES = _sizes()
THREE_SIZES = [7, 2451, SIZES[-1]]                      # a tail and one group; two workgroups; the capped grid


@pytest.fixture(scope="module")
def ops():
    from sfcvit import ops as o
    return o


def figure(what, **figures):
    print(f"FIGURE {what}: " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _dev(x, dtype=torch.float32):
    return torch.tensor(np.asarray(x), dtype=torch.float32).to("cuda", dtype=dtype)


def _state_buffer(lr=0.0, bc1=0.0, rbc2=0.0, step=0):
    """The int32[8] step state with [1] = step, [2..4] = the three floats, [5..7] a sentinel."""
    s = torch.zeros(8, dtype=torch.int32)
    s[1] = step
    s.view(torch.float32)[2:5] = torch.tensor([lr, bc1, rbc2], dtype=torch.float32)
    s[5:8] = 0x5A5A5A5A
    return s.cuda()


# ---- exact answers ------------------------------------------------------------------------------------------------------------
def run_design(ops, name, n, ema):
    """One launch of an exact design in guarded buffers.  -> ({output: elements differing from the closed form}, outputs)"""
    d = R.design(name, n)
    bufs = {k: guarded_inout(k, _dev(d[key])) for k, key in (("master", "w"), ("m", "m"), ("v", "v"))}
    bufs["param"] = guarded_inout("param", _dev(d["w"], BF16))
    bufs["grad"] = guarded_input("grad", _dev(d["g"], BF16))
    if ema:
        bufs["ema"] = guarded_inout("ema", torch.zeros(n, device="cuda"))
    state = sumsq = None
    if d["state"] is not None:
        bufs["state"] = guarded_inout("state", _state_buffer(*d["state"], step=1))
        state = bufs["state"].t
    if d["sumsq"] is not None:
        bufs["sumsq"] = guarded_input("sumsq", torch.tensor([d["sumsq"]], device="cuda"))
        sumsq = bufs["sumsq"].t
    state0 = state.clone() if state is not None else None
    args = [bufs[k].t for k in ("param", "master", "grad", "m", "v")] + [sumsq]
    if ema:
        ops.adamw_ema_step(*args, bufs["ema"].t, 0.5, False, dev_state=state, **d["hyper"])
    else:
        ops.adamw_step(*args, dev_state=state, **d["hyper"])
    torch.cuda.synchronize()
    want = {"master": _dev(d["want"]["w"]), "m": _dev(d["want"]["m"]), "v": _dev(d["want"]["v"])}
    want["param"] = want["master"].to(BF16)              # round to nearest even (adamw_ref.bf16_bits is held to it on the CPU)
    if ema:
        want["ema"] = _dev(d["want"]["ema"])
    diff = {k: int((_bits(bufs[k].t) != _bits(x)).sum()) for k, x in want.items()}
    diff["grad"] = int((_bits(bufs["grad"].t) != _bits(_dev(d["g"], BF16))).sum())       # an input: must not be written
    if state is not None:
        diff["state"] = int((state != state0).sum())
    assert_guards_intact(bufs.values(), f"{name} n={n} ema={ema}")
    return diff, {k: bufs[k].t.clone() for k in want}


@pytest.mark.parametrize("ema", [False, True], ids=["adamw_step", "adamw_ema_step"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", R.DESIGNS)
def test_exact_designs_bit_for_bit(ops, name, n, ema):
    """Both designs (the running one plain and with the clip's coefficient exactly 1) at every size of
    test_model_ema_gpu._sizes(), through adamw_step and adamw_ema_step: zero elements of master, m, v, ema and param differ
    from the closed form, the guards around every buffer are intact, and a second run gives the same bits."""
    diff, out = run_design(ops, name, n, ema)
    figure(f"exact {name} n={n} {'adamw_ema_step' if ema else 'adamw_step'} elements differing", **diff)
    diff2, out2 = run_design(ops, name, n, ema)
    rerun = sum(int((_bits(out[k]) != _bits(out2[k])).sum()) for k in out)
    figure(f"exact {name} n={n} second run", differing=rerun)
    assert all(c == 0 for c in diff.values()), diff
    assert diff2 == diff and rerun == 0
    if ema:
        assert ops.last_rowwise_kernel() == f"adamw_ema_kernel<{int(os.environ.get('SFCVIT_ADAMW_NT', '3')) & 3}>"


# ---- the fp64 bar over consecutive steps ----------------------------------------------------------------------------------------
def _unambiguous(w, dw):
    lo, hi = (w - dw).float().to(BF16), (w + dw).float().to(BF16)
    return _bits(lo) == _bits(hi)


@pytest.mark.parametrize("n", THREE_SIZES)
@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_four_steps_within_the_fp64_bar(ops, case, n):
    """K = 4 consecutive steps t0 .. t0 + 3 of a case (adamw_ref.CASES) from a random state (w ~ N(0, 1), m != 0, v from 1e-12
    to 1).  Each step's float64 reference starts from the state the kernel itself left, so the one-step bar holds at every
    step.  master, m and v within the bar; param bits = bf16 of the stored master, and of the reference master wherever the
    bar does not straddle a rounding boundary.  The largest size is compared on the device in float64 torch.  The clip's
    sum of squares is sumsq_accum's (read back: an input of the step); under dev_state the state is step_advance's, read
    back likewise."""
    t0, clip, gs, wd, lr, dev = case
    on_host = n <= 1 << 20
    seed = 5000 + 17 * R.CASES.index(case) + n % 1009
    w, m, v = (_dev(x) for x in R.random_state(n, seed))
    param = w.to(BF16)
    ss = torch.zeros(1, device="cuda") if clip else None
    state = _state_buffer(lr=lr, step=t0 - 1) if dev else None
    worst = dict(w=0.0, m=0.0, v=0.0)
    checked = 0
    for k in range(4):
        t = t0 + k
        grad = _dev(R.random_grad(n, seed + 1 + k, clip), BF16)
        st = sumsq = None
        if dev:
            ops.step_advance(state, R.BETA1, R.BETA2, 99)
            assert int(state[1]) == t
            st = state.view(torch.float32)[2:5].cpu().numpy()
        if clip:
            ss.zero_()
            ops.sumsq_accum(grad, ss)
            sumsq = float(ss)
            norm = sumsq ** 0.5 * gs
            assert (norm > 3.0) if clip == "binds" else (norm < 0.5), (clip, norm)
        before = [x.clone() for x in (w, m, v)]
        ops.adamw_step(param, w, grad, m, v, ss, lr=lr, beta1=R.BETA1, beta2=R.BETA2, eps=R.EPS, weight_decay=wd,
                       max_norm=R.MAX_NORM if clip else 0.0, step=t, grad_scale=gs, dev_state=state)
        kw, barkw = R.case_kwargs(case, t, sumsq, st)
        conv = (lambda x: x.float().cpu().numpy()) if on_host else (lambda x: x)
        ref = R.step64(*[conv(x) for x in before], conv(grad), **kw)
        bars = R.bar(ref[3], **barkw)
        for key, got, want, b in zip("wmv", (w, m, v), ref[:3], bars):
            worst[key] = max(worst[key], R.worst_ratio(conv(got), want, b))
        assert torch.equal(_bits(param), _bits(w.to(BF16))), (t, "param is not the bf16 rounding of the stored master")
        if on_host:
            sure = torch.from_numpy(R.bf16_unambiguous(ref[0], bars[0]))
            want_p = torch.from_numpy(R.bf16_bits(ref[0].astype(np.float32)).view(np.int16))
            wrong = int((_bits(param).cpu()[sure] != want_p[sure]).sum())
        else:
            sure = _unambiguous(ref[0], bars[0])
            wrong = int((_bits(param)[sure] != _bits(ref[0].float().to(BF16))[sure]).sum())
        checked += int(sure.sum())
        assert wrong == 0, (t, wrong, "param differs from the bf16 rounding of the reference master")
        assert not torch.equal(before[0], w)
    figure(f"bar {R.CASE_IDS[R.CASES.index(case)]} n={n} worst |err|/bar over 4 steps", **worst, param_checked_against_reference=checked)
    assert max(worst.values()) <= 1.0
    assert checked >= 3 * n


# ---- edge elements ------------------------------------------------------------------------------------------------------------
def test_edge_elements_planted_in_one_vector(ops):
    """adamw_ref.edge_vector(): g = 0 with v = 0 (eps 1e-8: only the decay moves w), w = -0.0, subnormal v, a gradient whose
    square is subnormal or underflows, g = +-3e38 whose square overflows (v = inf, update 0).  The state (lr, bc1, rbc2) is
    written by the test, so the kernel's inputs are known exactly.  Reference: step32 under every combination of
    contraction choices (adamw_ref.all_contractions, which contain the issue's two variants): where they all agree the kernel
    must give those bits, elsewhere it is held to the bar against step64 -- and every element's bits must be those of SOME
    combination: a correctly rounded evaluation of the step.  (Agreement of the all-fused-right and the unfused variant alone
    is not enough for a bit comparison: on one element of this vector those two agree while fma(decay, w, -fl(c q)), which the
    compiler emits and which is as correct, rounds the other way.)  Printed besides: which combinations explain the whole
    vector."""
    w0, m0, v0, g0, where = R.edge_vector()
    n = w0.size
    lr, bc1, rbc2 = R.edge_state32()
    state = _state_buffer(float(lr), float(bc1), float(rbc2), step=R.EDGE_STEP)
    bufs = {k: guarded_inout(k, _dev(x)) for k, x in (("master", w0), ("m", m0), ("v", v0))}
    bufs["param"] = guarded_inout("param", _dev(w0, BF16))
    bufs["grad"] = guarded_input("grad", _dev(g0, BF16))
    assert torch.equal(_bits(bufs["master"].t.cpu()), torch.from_numpy(w0.view(np.int32))), "the upload must keep -0.0 and subnormals"
    assert torch.equal(_bits(bufs["v"].t.cpu()), torch.from_numpy(v0.view(np.int32)))
    ops.adamw_step(*[bufs[k].t for k in ("param", "master", "grad", "m", "v")], None, lr=55.0, max_norm=0.0, step=R.EDGE_STEP,
                   dev_state=state, **{k: x for k, x in R.EDGE_HYPER.items() if k != "lr"})
    torch.cuda.synchronize()
    assert_guards_intact(bufs.values(), "edge vector")
    kw = dict(R.EDGE_HYPER, bc1=bc1, rbc2=rbc2)
    kw["lr"] = lr
    combos = R.all_contractions()
    outs = [R.step32(w0, m0, v0, g0, contract=c, **kw) for c in combos]
    with np.errstate(all="ignore"):
        ref = R.step64(w0, m0, v0, g0, **kw)
        bars = R.bar(ref[3], clip=False)
    got = [bufs[k].t.cpu().numpy() for k in ("master", "m", "v")]
    agree = np.ones(n, dtype=bool)
    same = []                                            # per combination: the elements on which the kernel has its bits
    for o in outs:
        hit = np.ones(n, dtype=bool)
        for a, b, x in zip(o, outs[0], got):
            agree &= a.view(np.uint32) == b.view(np.uint32)
            hit &= a.view(np.uint32) == x.view(np.uint32)
        same.append(hit)
    whole = [c for c, hit in zip(combos, same) if hit.all()]
    print("contractions that give the kernel's bits on every element:", len(whole), "of", len(combos), "e.g.", whole[:1],
          "; the all-left one (LLVM's) does:", R.contraction(True) in whole)
    differing = {k: int((a.view(np.uint32) != b.view(np.uint32))[agree].sum()) for k, a, b in zip(("master", "m", "v"), got, outs[0])}
    worst = max([R.worst_ratio(a[~agree], b[~agree], c[~agree]) for a, b, c in zip(got, ref[:3], bars)]) if (~agree).any() else 0.0
    for name, ps in where.items():
        for p in ps:
            print(f"edge {name} [{p}]: w {w0[p]!r} -> {got[0][p]!r}  m -> {got[1][p]!r}  v -> {got[2][p]!r}  (step32: {outs[0][0][p]!r} "
                  f"{outs[0][1][p]!r} {outs[0][2][p]!r})")
    figure("edge vector", elements=n, variants_agree=int(agree.sum()), **{f"{k}_differing_there": c for k, c in differing.items()},
           worst_ratio_elsewhere=float(worst), elements_some_contraction_explains=int(np.any(same, axis=0).sum()),
           contractions_explaining_all=len(whole), llvm_left_explains_all=R.contraction(True) in whole)
    special = [p for k in ("g0_v0", "g0_v0_negzero_w", "g_+3e38", "g_-3e38") for p in where[k]]
    assert agree[special].all()
    assert all(c == 0 for c in differing.values()), differing
    assert worst <= 1.0
    assert np.any(same, axis=0).all(), "an element's bits are no correctly rounded evaluation of the step under any contraction"
    assert all(got[0][p].view(np.uint32) == 0x80000000 for p in where["g0_v0_negzero_w"])
    assert all(np.isinf(got[2][p]) for p in where["g_+3e38"] + where["g_-3e38"])
    assert torch.equal(_bits(bufs["param"].t), _bits(bufs["master"].t.to(BF16)))


# ---- step_advance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start,count", [(0, 5), (999, 1)], ids=["steps-1-to-5", "step-1000"])
def test_step_advance_against_the_restatement(ops, start, count):
    """Counter and seed offset bit for bit; state[3] = 1 - beta1^t and state[4] = 1 / sqrt(1 - beta2^t) against float64 by
    adamw_ref.advance_bar (which allows the device powf adamw_ref.DEVICE_POWF_ULPS ulp, an allowance taken from the OpenCL
    full profile, not measured: the observed error is printed); state[2] (the host's lr) and state[5..7] untouched."""
    seed_base = 0xDEADBEEF if start else 4242
    buf = guarded_inout("state", _state_buffer(lr=3e-4, step=start))
    s0 = buf.t.clone().cpu()
    for step in range(start + 1, start + count + 1):
        ops.step_advance(buf.t, R.BETA1, R.BETA2, seed_base)
        torch.cuda.synchronize()
        s = buf.t.cpu()
        want_step, off, bc1, rbc2 = R.advance_ref(step - 1, R.BETA1, R.BETA2, seed_base)
        f = s.view(torch.float32)
        b1, b2 = R.advance_bar(R.BETA1, R.BETA2, step)
        r1, r2 = abs(float(f[3]) - bc1) / b1, abs(float(f[4]) - rbc2) / b2
        figure(f"step_advance step {step}", counter=int(s[1]), offset=f"{int(s[0]) & 0xFFFFFFFF:#010x}", want_offset=f"{off:#010x}",
               bc1_ratio=float(r1), rbc2_ratio=float(r2), powf_beta1_ulps=float(R.powf_ulps(float(f[3]), R.BETA1, step)))
        assert int(s[1]) == want_step == step and int(s[0]) & 0xFFFFFFFF == off
        assert r1 <= 1.0 and r2 <= 1.0
        assert int(s[2]) == int(s0[2]) and torch.equal(s[5:8], s0[5:8])
    assert_guards_intact([buf], "step_advance")


# ---- non-finite gradients -------------------------------------------------------------------------------------------------------
NF_HYPER = dict(lr=1e-3, beta1=R.BETA1, beta2=R.BETA2, eps=R.EPS, weight_decay=5e-2)
NF_N, NF_AT, NF_STEP = 1031, 517, 3


def _nf_run(ops, grad, clip, state):
    w, m, v = (_dev(x) for x in state)
    param = w.to(BF16)
    ss = None
    if clip:
        ss = torch.zeros(1, device="cuda")
        ops.sumsq_accum(grad, ss)
    ops.adamw_step(param, w, grad, m, v, ss, max_norm=R.MAX_NORM if clip else 0.0, step=NF_STEP, **NF_HYPER)
    return dict(master=w, m=m, v=v, param=param), (float(ss) if clip else None)


@pytest.mark.parametrize("clip", [False, True], ids=["no-clip", "clip"])
@pytest.mark.parametrize("kind", ["inf", "nan"])
def test_non_finite_gradient_is_not_swallowed(ops, kind, clip):
    """One inf, or one NaN, among 1030 finite gradients (norm >> max_norm).  Pinned:

    the element itself      master and param end NaN in all four cases (m, v: NaN; inf, inf without the clip under an inf
                            gradient) -- never a finite weight.
    the other elements      without the clip: exactly the step they take when that gradient is 0 (bit for bit).
                            inf under the clip: the norm is inf, the coefficient max_norm / inf = 0, every finite gradient is
                            scaled to 0: exactly the step of an all-zero gradient (decay and the old momentum only).
                            NaN under the clip: fminf(1, max_norm / NaN) returns 1 (IEEE minimum ignores a quiet NaN), so the
                            finite elements take exactly the UNCLIPPED step.

    torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW on the same gradient (computed below on the CPU, one step from zero
    moments): without the clip, and for inf under the clip (coefficient 0, inf * 0 = NaN), only that element turns NaN, as
    here.  For NaN under the clip torch's coefficient is NaN and EVERY parameter turns NaN, where this kernel steps the
    finite elements unclipped: a documented difference in the finite elements, left as it is.  The poisoned element cannot
    be missed in either."""
    bad = float(kind)
    state = R.random_state(NF_N, 900)
    g = R.random_grad(NF_N, 901, "binds")
    g_bad = g.copy()
    g_bad[NF_AT] = bad
    g_zeroed = g.copy()
    g_zeroed[NF_AT] = 0.0
    got, sumsq = _nf_run(ops, _dev(g_bad, BF16), clip, state)
    if not clip or kind == "nan":
        twin, _ = _nf_run(ops, _dev(g_zeroed, BF16), False, state)          # unclipped, that gradient 0
    else:
        twin, _ = _nf_run(ops, torch.zeros(NF_N, device="cuda", dtype=BF16), False, state)
    others = torch.ones(NF_N, dtype=torch.bool, device="cuda")
    others[NF_AT] = False
    moved = {k: int((_bits(got[k]) != _bits(twin[k]))[others].sum()) for k in got}
    nonfinite_others = int((~torch.isfinite(got["master"]))[others].sum())
    at = {k: float(got[k][NF_AT]) for k in got}
    # torch on the CPU, for the record in the docstring
    p = torch.nn.Parameter(torch.from_numpy(state[0].copy()))
    p.grad = torch.from_numpy(g_bad.copy())
    if clip:
        torch.nn.utils.clip_grad_norm_([p], R.MAX_NORM)
    torch.optim.AdamW([p], lr=NF_HYPER["lr"], betas=(R.BETA1, R.BETA2), eps=R.EPS, weight_decay=NF_HYPER["weight_decay"]).step()
    torch_nonfinite = int((~torch.isfinite(p.detach())).sum())
    figure(f"non-finite {kind} {'clip' if clip else 'no-clip'}", sumsq=str(sumsq), master_at=str(at["master"]), param_at=str(at["param"]),
           m_at=str(at["m"]), v_at=str(at["v"]), others_nonfinite=nonfinite_others,
           **{f"others_differing_from_twin_{k}": c for k, c in moved.items()}, torch_nonfinite_params=torch_nonfinite)
    assert np.isnan(at["master"]) and np.isnan(at["param"]), at              # never a finite weight from a non-finite gradient
    assert not np.isfinite(at["m"]) and not np.isfinite(at["v"])
    assert nonfinite_others == 0 and all(c == 0 for c in moved.values()), moved
    assert torch_nonfinite == (NF_N if (clip and kind == "nan") else 1)
    assert bool(torch.isnan(p.detach()[NF_AT]))
    if clip:
        assert sumsq is not None and not np.isfinite(sumsq)


# ---- the other template instances -----------------------------------------------------------------------------------------------
def child():
    """SFCVIT_ADAMW_NT is read once per process: this runs in a fresh one (test_other_instances_in_fresh_processes) and prints
    the differing-element counts of the exact designs at THREE_SIZES through both kernels."""
    from sfcvit import ops
    print("CHILD NT", os.environ.get("SFCVIT_ADAMW_NT"))
    for name in R.DESIGNS:
        for n in THREE_SIZES:
            for ema in (False, True):
                diff, _ = run_design(ops, name, n, ema)
                last = ops.last_rowwise_kernel() if ema else "-"
                print(f"CHILD {name} n={n} ema={int(ema)} differing={sum(diff.values())} kernel={last}")
    torch.cuda.synchronize()
    print("CHILD ok")


@pytest.mark.parametrize("nt", ["0", "1", "2"])
def test_other_instances_in_fresh_processes(nt):
    """adamw_kernel<0|1|2> and adamw_ema_kernel<0|1|2> (plain or non-temporal loads / stores): a fresh child process per
    value of SFCVIT_ADAMW_NT runs the exact designs at 7, 2451 and the capped size; zero differing elements, and the EMA
    call reports the instance asked for."""
    env = dict(os.environ, SFCVIT_ADAMW_NT=nt)
    code = (f"import sys; sys.path[:0] = [{TESTS!r}, {ROOT!r}, {PKG!r}]; "
            "import test_adamw_edges_gpu as t; t.child()")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "CHILD ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = re.findall(r"^CHILD (\S+) n=(\d+) ema=(\d) differing=(\d+) kernel=(\S+)$", r.stdout, re.M)
    figure(f"SFCVIT_ADAMW_NT={nt}", runs=len(lines), differing=sum(int(x[3]) for x in lines),
           ema_kernels=",".join(sorted({x[4] for x in lines if x[2] == "1"})))
    assert f"CHILD NT {nt}" in r.stdout
    assert len(lines) == len(R.DESIGNS) * len(THREE_SIZES) * 2
    assert all(int(x[3]) == 0 for x in lines), lines
    assert all(x[4] == f"adamw_ema_kernel<{nt}>" for x in lines if x[2] == "1"), lines
