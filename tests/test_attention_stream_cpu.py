"""Any-length attention without a GPU: which kernels sfcvit_attention_plan (host only) selects for the any-length entry
points, and the resource usage of the streaming head-dim 128 / 192 / 256 kernels as hipcc compiles them for gfx950."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd", "csrc")
SWITCH = "SFCVIT_ATTN_WIDE_STREAM"


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in (SWITCH, "SFCVIT_ATTN_LONG", "SFCVIT_ATTN_BWD_FUSED", "SFCVIT_ATTN_DQSUM", "SFCVIT_ATTN_BWD_PERSIST"):
        monkeypatch.delenv(name, raising=False)


def plan(B, N, H, hd, bwd, any_length, p=0.0):
    """(status, kernel name or error message) of one attention call, planned on the host."""
    from sfcvit import _lib
    a = _lib.AttnArgs()
    a.qkv, a.out, a.lse, a.dout, a.dqkv, a.delta = (0x100000 * (i + 1) for i in range(6))   # checked, never read
    a.B, a.N, a.H, a.hd, a.scale, a.dropout_p = B, N, H, hd, hd ** -0.5, p
    buf = ctypes.create_string_buffer(96)
    rc = _lib.lib.sfcvit_attention_plan(ctypes.byref(a), int(bwd), int(any_length), buf, len(buf))
    return (rc, _lib.lib.sfcvit_last_error().decode()) if rc else (0, buf.value.decode())


# csrc/hostcheck/host_check.cpp's wide-head rows: (B, N, H, hd, p, bwd) -> kernel, or a fragment of the refusal
WIDE_ROWS = [
    ((8, 196, 4, 128, 0.0, False), "attn_wide_fwd_kernel<2>"),
    ((8, 196, 4, 128, 0.1, True), "attn_wide_bwd_kv_kernel<2>"),
    ((8, 128, 4, 192, 0.0, False), "attn_wide_fwd_kernel<3>"),
    ((8, 128, 4, 256, 0.0, True), "attn_wide_bwd_kv_kernel<4>"),
    ((8, 196, 4, 192, 0.0, False), "attention: head dim 192 with N = 196 needs 168 KiB of LDS"),
    ((8, 196, 4, 256, 0.0, True), "attention: head dim 256 with N = 196 needs 226 KiB of LDS"),
    ((8, 300, 4, 128, 0.0, False), "attention: head dim 128 with N = 300 needs"),
    ((8, 196, 4, 96, 0.0, False), "attention_fwd: head dim 96 not supported"),
]

# head dim 64: ViT-B at batch 256 / 64, ViT-L/16 @ 384, ViT-Tiny @ 32, the two-kernel backward range, the tiled range
HD64 = [(256, 196, 12, 64), (64, 196, 12, 64), (64, 576, 16, 64), (64, 577, 16, 64), (256, 4, 3, 64), (8, 240, 4, 64),
        (8, 1024, 4, 64), (2, 3136, 2, 64)]


@pytest.mark.parametrize("shape,want", WIDE_ROWS)
def test_default_entry_points_keep_todays_plan(shape, want):
    B, N, H, hd, p, bwd = shape
    rc, got = plan(B, N, H, hd, bwd, any_length=False, p=p)
    if want.startswith("attention"):
        assert rc == 1 and want in got, (rc, got)
    else:
        assert (rc, got) == (0, want)


@pytest.mark.parametrize("B,N,H,hd", [(8, 196, 4, 192), (8, 300, 4, 128), (1, 3136, 4, 192), (8, 196, 4, 256),
                                      (2, 257, 1, 128), (64, 576, 8, 128)])
@pytest.mark.parametrize("bwd", [False, True])
def test_any_length_streams_where_the_whole_sequence_kernels_refuse(B, N, H, hd, bwd):
    rc, msg = plan(B, N, H, hd, bwd, any_length=False)
    assert rc == 1 and "LDS" in msg
    want = f"attn_wide_stream_{'bwd_kv' if bwd else 'fwd'}_kernel<{hd // 64}>"
    assert plan(B, N, H, hd, bwd, any_length=True) == (0, want)
    assert plan(B, N, H, hd, bwd, any_length=True, p=0.1) == (0, want)


@pytest.mark.parametrize("shape,want", WIDE_ROWS[:4])
def test_any_length_keeps_the_whole_sequence_kernels_where_they_fit(shape, want):
    B, N, H, hd, p, bwd = shape
    assert plan(B, N, H, hd, bwd, any_length=True, p=p) == (0, want)


@pytest.mark.parametrize("B,N,H,hd", HD64)
@pytest.mark.parametrize("bwd", [False, True])
def test_head_dim_64_selects_what_it_selects_today(monkeypatch, B, N, H, hd, bwd):
    for p in (0.0, 0.1):
        today = plan(B, N, H, hd, bwd, any_length=False, p=p)
        assert today[0] == 0 and "stream" not in today[1]
        assert plan(B, N, H, hd, bwd, any_length=True, p=p) == today
        monkeypatch.setenv(SWITCH, "1")                          # the switch concerns head dims > 64 only
        assert plan(B, N, H, hd, bwd, any_length=True, p=p) == today
        monkeypatch.delenv(SWITCH)


def test_head_dim_96_is_still_refused():
    """Padding 96 to 128 is the op level's business (functional.py), not the C ABI's."""
    for bwd in (False, True):
        rc, msg = plan(8, 196, 4, 96, bwd, any_length=True)
        assert rc == 1 and "head dim 96 not supported" in msg


def test_switch_forces_streaming_for_any_length_calls_only(monkeypatch):
    monkeypatch.setenv(SWITCH, "1")                              # read per call
    for N in (1, 5, 64, 196):
        assert plan(2, N, 2, 128, False, any_length=True) == (0, "attn_wide_stream_fwd_kernel<2>")
        assert plan(2, N, 2, 192, True, any_length=True) == (0, "attn_wide_stream_bwd_kv_kernel<3>")
        assert plan(2, N, 2, 128, False, any_length=False) == (0, "attn_wide_fwd_kernel<2>")
    monkeypatch.setenv(SWITCH, "0")
    assert plan(2, 196, 2, 128, False, any_length=True) == (0, "attn_wide_fwd_kernel<2>")


def test_plan_refuses_bad_arguments_with_a_message():
    from sfcvit import _lib
    buf = ctypes.create_string_buffer(96)
    assert _lib.lib.sfcvit_attention_plan(None, 0, 1, buf, len(buf)) == 1
    a = _lib.AttnArgs()                                          # null tensors
    a.B, a.N, a.H, a.hd = 1, 16, 1, 128
    assert _lib.lib.sfcvit_attention_plan(ctypes.byref(a), 0, 1, buf, len(buf)) == 1
    assert b"null" in _lib.lib.sfcvit_last_error()


def _stream_lds(S, kv):
    """Dynamic LDS of a STREAM kernel (csrc/dispatch.h, stream_lds): two 64-row blocks of S images with 128-byte rows,
    + lse / delta / mask row key of 64 rows in the dK / dV kernel."""
    return 2 * S * 64 * 128 + (3 * 64 * 4 if kv else 0)


def test_streaming_kernels_use_no_scratch_and_fit_twice_per_cu(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(CSRC, "attention_wide_stream.hip")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--offload-device-only", "-ffp-contract=fast",
           "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "stream.co")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-4000:]
    # per kernel: "remark: Function Name: <mangled> [...]", then lines "remark:     <field>: <value> [...]"
    fields = {"ScratchSize [bytes/lane]": "scratch", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill",
              "LDS Size [bytes/block]": "lds"}
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(.+?): (\d+) ", line)
        if m and cur is not None and m.group(1) in fields:
            cur[fields[m.group(1)]] = int(m.group(2))
    seen = set()
    for name, res in kernels.items():
        m = re.search(r"attn_wide_stream_(fwd|bwd_kv|bwd_q)_kernelILi(\d)E", name)
        if not m:
            continue
        kind, S = m.group(1), int(m.group(2))
        seen.add((kind, S))
        assert res.get("scratch") == 0 and res.get("vgpr_spill") == 0 and res.get("sgpr_spill") == 0, (name, res)
        lds = res["lds"] + _stream_lds(S, kind == "bwd_kv")
        assert 2 * lds <= 160 * 1024, (name, lds)
    assert seen == {(kind, S) for kind in ("fwd", "bwd_kv", "bwd_q") for S in (2, 3, 4)}, sorted(seen)
