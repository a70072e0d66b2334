// Kernel selection of sfcvit_gemm and sfcvit_attention_fwd / _bwd (dispatch.h): argument checks, family, template
// instance, grid and post passes.  Plain host code: no HIP call, no allocation, no lock.
#include "dispatch.h"

#include <cstdint>
#include <cstdio>

namespace sfcvit {
namespace {

// The persistent 8-phase kernel (gemm8p.hip): false when the shape / options are not eligible.
bool plan_p8(GemmPlan &p, const sfcvit_gemm_args &a, int splits, int cus, const Knobs &k) {
    if (a.a_kmajor || a.b_kmajor || splits != 1 || a.c_is_f32 || a.aux_out) return false;
    if (a.act == SFCVIT_ACT_GELU || a.dact == SFCVIT_ACT_GELU) return false;
    if (a.N % 256 || a.K % 128 || a.K < 256 || a.lda % 8 || a.ldb % 8 || a.ldc % 8) return false;
    if (a.lda >= (1 << 21) || a.ldb >= (1 << 21)) return false;       // 32-bit byte offsets within a tile
    if (a.M / 192 >= 32768 || a.N / 256 >= 65536) return false;       // (row tile, column tile) packed into one int
    if (a.residual && (a.ldr % 8 || !aligned(a.residual, 16))) return false;
    if (a.dact && (a.ldaux % 8 || !aligned(a.aux_in, 16))) return false;
    if (a.bias && !aligned(a.bias, 16)) return false;
    int mask = 0;
    if (a.act == SFCVIT_ACT_RELU) mask |= P8_RELU;
    if (a.dropout_p > 0.f) mask |= P8_DROP;
    if (a.residual) mask |= P8_RES;
    if (a.dact == SFCVIT_ACT_RELU) mask |= P8_DACT;
    if (a.colsum_out) mask |= P8_CSUM;
    if (a.actmask && (mask & (P8_RELU | P8_DACT)) && !(mask & P8_RES)) mask |= P8_BITS;   // with RELU + RES the bits come from the pass over C
    if ((mask & P8_DACT) && a.bias) return false;                // the DACT variants leave the bias out (register room)
    if (a.bias && a.N > BIAS_MAX_N) return false;
    switch (mask) {                                              // the instantiated epilogues (CSUM only with DACT)
    case 0: case P8_RES: case P8_DROP | P8_RES: case P8_RELU: case P8_RELU | P8_DROP: case P8_DACT: case P8_DACT | P8_CSUM:
    case P8_RELU | P8_BITS: case P8_RELU | P8_DROP | P8_BITS: case P8_DACT | P8_BITS: case P8_DACT | P8_CSUM | P8_BITS: break;
    default: return false;
    }
    const int grid = cus / 8 * 8;
    if (grid < 8) return false;
    // Tile height: the one whose rounds of tiles cost least.  A tile's time is not proportional to its rows: the stamped
    // k-tile (profiles/r3/gemm8p_ktile_trace.txt) takes 2 663 clocks at 256 rows and 2 487 at 224 (0.934, not 0.875) -- the
    // per-section hand-off does not shrink with the tile; 192 rows extrapolated.  With these weights N = 3 072 at M = 50 176
    // takes 256-row tiles (10 rounds x 1 000 < 11 x 934; measured 234 vs 238 us and 219 vs 226 us), N = 768 stays at 224.
    // Any M >= one tile: a height that does not divide M makes the last row tile overlap its predecessor (kernel header),
    // which costs that tile's share of recomputed rows, i.e. it is priced as one more tile.  The overlapping tile reads
    // residual / aux_in rows another workgroup may be storing to if C aliases them: refused then.
    const int nt = a.N / 256;
    const bool aliased = a.c == a.residual || a.c == a.aux_in;
    long best = -1;
    int ni = 0;
    for (int cand : {8, 7, 6}) {
        if (a.M < 32 * cand || (a.M % (32 * cand) && aliased)) continue;
        const long tiles = long((a.M + 32 * cand - 1) / (32 * cand)) * nt;
        const long cost = ((tiles + grid - 1) / grid) * (cand == 8 ? 1000 : cand == 7 ? 934 : 870);
        if (best < 0 || cost < best) { best = cost; ni = cand; }
    }
    if (!ni) return false;
    const int pinned = a.force_generic == SFCVIT_GEMM_P8_256 ? 8 : a.force_generic == SFCVIT_GEMM_P8_224 ? 7
                     : a.force_generic == SFCVIT_GEMM_P8_192 ? 6 : 0;      // tests: pin the tile height
    if (pinned) {
        if (a.M < 32 * pinned || (a.M % (32 * pinned) && aliased)) return false;
        ni = pinned;
    }
    const int nparts = 2 * ((a.M + 32 * ni - 1) / (32 * ni));    // CSUM: one partial row per (row tile, wave group)
    if (mask & P8_CSUM) {
        const int64_t need = int64_t(nparts) * a.N * int64_t(sizeof(float));
        if (!a.workspace || a.workspace_bytes < need || !aligned(a.workspace, 16)) return false;
        p.colsum_parts = nparts;
    }
    p.family = GemmFamily::P8;
    p.ni = ni;
    p.mask = mask;
    p.p2 = k.gemm_2phase;
    p.grid = grid;
    // Tile walk: column windows of 6 tiles for the wide GEMMs (N >= 1 792).  An XCD's 32 concurrent tiles are then ~5 row
    // tiles x 6 column tiles instead of ~3 x 9-12, i.e. 11 distinct operand panels instead of 12-15: memory-side fetch of the
    // N = 3 072 / 2 304 forward GEMMs 427 -> 263 MB per launch, L2 hit rate 0.56 -> 0.63, time unchanged
    // (profiles/r4/gemm_tile_walk_ab.txt).
    p.walk = k.gemm_walk >= 0 ? k.gemm_walk : (a.N / 256 > 6 ? 6 : 0);
    // Start-up stagger: the 32 workgroups of an XCD start in 4 groups 2 us apart.  Uniform tiles keep the 256 workgroups of a
    // launch in lockstep, so all of them reach their epilogue in the same microsecond and 33 MB of C hit the memory system at
    // once (the epilogue section of the first tiles of a launch takes 10 000 clocks, 5 600 once the workgroups have drifted
    // apart: profiles/r3/gemm8p_ktile_trace.txt); the tile queue absorbs the late starts (late workgroups draw fewer tiles).
    // Measured alone, M = 50 176 (tools/gemm_lab/ab_two_phase.py with AB_STAGGER): QKV 148.9 -> 141.7 us, out-proj 74.4 ->
    // 68.6, linear1 233.7 -> 230.9, linear2 208.0 -> 205.3, linear2 dX 225.8 -> 221.4, linear1 dX 206.6 -> 203.1, in_proj dX
    // 162.0 -> 161.6; training step 33.26-33.38 -> 32.86-32.89 ms (three alternating pairs of runs on one box).
    // A launch whose workgroups draw one tile each has no lockstep to break: the delay would only lengthen it.
    p.stag_slots = k.gemm_stagger_slots < 1 ? 1 : k.gemm_stagger_slots;
    p.stag_ticks = long((a.M + 32 * ni - 1) / (32 * ni)) * nt < 2L * grid ? 0 : k.gemm_stagger_ticks;
    return true;
}

// Weight-gradient form of the persistent kernel (both operands k-major, split-K into the workspace slabs).  k need not be a
// multiple of 128 (k = batch x tokens: 19 600 rows at batch 100): the kernel takes the largest multiple and the remaining
// < 128 rows are one more slab from the generic kernel (a slab is kept free for it), summed with the others in the same
// fixed order.
bool plan_p8_km(GemmPlan &p, const sfcvit_gemm_args &a, int splits_req, int cus, const Knobs &k) {
    if (!a.a_kmajor || !a.b_kmajor || splits_req < 2) return false;
    if (a.M % 256 || a.N % 256 || a.K < 256 || a.lda % 8 || a.ldb % 8) return false;
    if (!cus) return false;
    const int Kb = a.K / 128 * 128, tail = a.K - Kb;
    const int tiles = (a.M / 256) * (a.N / 256), KT = Kb / 64;
    // SFCVIT_RESERVE_CUS=n: leave n CUs out of the split, for nodes where collectives run beside backward -- a launch of one
    // workgroup per CU takes twice as long when it does not fit on the CUs that are free
    const int reserve = k.reserve_cus < 0 || k.reserve_cus > cus / 2 ? 0 : k.reserve_cus;
    int splits = (cus - reserve) / tiles;                         // one workgroup per CU
    if (splits > splits_req) splits = splits_req;
    const int64_t slabs_avail = a.workspace_bytes / (int64_t(a.M) * a.N * int64_t(sizeof(float))) - (tail ? 1 : 0);
    if (splits > slabs_avail) splits = int(slabs_avail);
    if (splits < 2) return false;
    const int kps = ((KT + splits - 1) / splits + 1) / 2 * 2;    // k-tiles per split, even
    splits = (KT + kps - 1) / kps;
    if (splits < 2) return false;
    p.family = GemmFamily::P8_KM;
    p.p2 = k.gemm_2phase;
    p.grid = (tiles * splits + 7) / 8 * 8;
    p.splits = splits;
    p.k_per_split = kps;
    p.k_done = Kb;
    p.tail_slab = tail ? splits : -1;
    p.reduce_slabs = splits + (tail ? 1 : 0);
    return true;
}

// The LDS-DMA ring kernel (gemm256.hip).
bool plan_ring(GemmPlan &p, const sfcvit_gemm_args &a, int splits, int k_per_split) {
    if (a.M % 256 || a.N % 128 || a.K % 32 || k_per_split % 32) return false;
    // BN = 256 unless that leaves the last round of workgroups mostly idle on 256 CUs.
    bool bn256 = a.N % 256 == 0;
    if (bn256) {
        const long t = long(a.M / 256) * (a.N / 256) * splits;
        const long rounds = (t + 255) / 256;
        if (t < 200 || double(t) / double(rounds * 256) < 0.85) bn256 = false;
    }
    // Measured on the ViT-B shapes (tools/bench_gemm.py, profiles/r1): the 256 x 128 two-workgroup
    // configuration wins when both operands are k-contiguous (forward GEMMs: 730-880 TFLOP/s vs
    // 650-760 generic, 650-820 for 256 x 256); with a k-major operand (dX, dW: transposed LDS reads,
    // twice the LDS instructions) the generic kernel's 128 x 128 tiles are as fast or faster.
    if (a.force_generic == SFCVIT_GEMM_AUTO) {
        if (a.a_kmajor || a.b_kmajor) return false;
        bn256 = false;
    }
    if (a.force_generic == SFCVIT_GEMM_RING_256x128) bn256 = false;
    if (a.force_generic == SFCVIT_GEMM_RING_256x256 && a.N % 256 == 0) bn256 = true;
    p.family = GemmFamily::RING;
    p.bn = bn256 ? 256 : 128;
    p.grid = (a.M / 256) * (a.N / p.bn);
    return true;
}

}  // namespace

GemmPlan gemm_plan(const sfcvit_gemm_args &a, int cus, const Knobs &k) {
    GemmPlan p;                                                  // (sfcvit_gemm has checked colsum_out and its workspace)
    if (a.actmask) {
        if (a.N % 16 || a.ld_actmask % 2 || a.ld_actmask * 8 < a.N || !aligned(a.actmask, 2))
            REFUSE(SFCVIT_EINVAL, "gemm: actmask needs N %% 16 == 0, an even ld_actmask >= N / 8 and 2-byte alignment");
        if (a.act != SFCVIT_ACT_RELU && a.dact != SFCVIT_ACT_RELU)
            REFUSE(SFCVIT_EINVAL, "gemm: actmask goes with act = RELU (written) or dact = RELU (read)");
        if (a.c_is_f32 || a.splitk > 1) REFUSE(SFCVIT_EINVAL, "gemm: actmask not with fp32 C or split-K");
    }
    if (!a.a || !a.b || !a.c) REFUSE(SFCVIT_EINVAL, "gemm: null operand");
    if (a.M <= 0 || a.N <= 0 || a.K <= 0) REFUSE(SFCVIT_EINVAL, "gemm: M=%d N=%d K=%d", a.M, a.N, a.K);
    // 16-byte vectors along the contiguous dimension of every operand.
    if (a.K % 8 != 0 && (!a.a_kmajor || !a.b_kmajor))
        REFUSE(SFCVIT_EINVAL, "gemm: K=%d must be a multiple of 8 for a k-contiguous operand", a.K);
    if (a.a_kmajor && a.M % 8 != 0) REFUSE(SFCVIT_EINVAL, "gemm: M=%d must be a multiple of 8 for k-major A", a.M);
    if ((a.b_kmajor && a.N % 8 != 0) || a.N % 4 != 0) REFUSE(SFCVIT_EINVAL, "gemm: N=%d must be a multiple of 4 (8 for k-major B)", a.N);
    if (a.lda % 8 || a.ldb % 8 || a.ldc % 4) REFUSE(SFCVIT_EINVAL, "gemm: lda=%d ldb=%d ldc=%d alignment", a.lda, a.ldb, a.ldc);
    if (!aligned(a.a, 16) || !aligned(a.b, 16) || !aligned(a.c, 16)) REFUSE(SFCVIT_EINVAL, "gemm: operands must be 16-byte aligned");
    if (a.residual && (a.ldr % 4 || !aligned(a.residual, 8))) REFUSE(SFCVIT_EINVAL, "gemm: residual alignment");
    if ((a.aux_in || a.aux_out) && a.ldaux % 4) REFUSE(SFCVIT_EINVAL, "gemm: ldaux=%d alignment", a.ldaux);
    if (a.dact != SFCVIT_ACT_NONE && !a.aux_in) REFUSE(SFCVIT_EINVAL, "gemm: dact needs aux_in");
    if (a.act < 0 || a.act > 2 || a.dact < 0 || a.dact > 2) REFUSE(SFCVIT_EINVAL, "gemm: bad act/dact");
    if (a.bias && !aligned(a.bias, 8)) REFUSE(SFCVIT_EINVAL, "gemm: bias alignment");
    if (!(a.dropout_p >= 0.f && a.dropout_p < 1.f)) REFUSE(SFCVIT_EINVAL, "gemm: dropout_p=%g out of [0, 1)", a.dropout_p);
    int splits = a.splitk < 1 ? 1 : a.splitk;
    const int ktiles = (a.K + GEN_BK - 1) / GEN_BK;
    if (splits > ktiles) splits = ktiles;
    const int out_tiles = ((a.N + GEN_TILE - 1) / GEN_TILE) * ((a.M + GEN_TILE - 1) / GEN_TILE);
    const bool per_xcd = splits > 1 && out_tiles < 64;          // one set of k-ranges per XCD (see gemm_kernel)
    if (per_xcd) splits = (splits + 7) / 8 * 8;
    const int k_per_split = ((ktiles + splits - 1) / splits) * GEN_BK;
    if (!per_xcd) splits = (a.K + k_per_split - 1) / k_per_split;   // drop empty trailing ranges
    if (splits > 1) {
        if (a.bias || a.residual || a.aux_out || a.act || a.dact || a.dropout_p > 0.f)
            REFUSE(SFCVIT_EINVAL, "gemm: split-K supports no epilogue");
        const int64_t need = int64_t(splits) * a.M * a.N * int64_t(sizeof(float));
        if (!a.workspace || a.workspace_bytes < need || !aligned(a.workspace, 16))
            REFUSE(SFCVIT_EINVAL, "gemm: split-K workspace too small (%lld bytes needed; use sfcvit_gemm_workspace)", (long long)need);
    }

    const int fg = a.force_generic;
    p.a_km = a.a_kmajor != 0;
    p.b_km = a.b_kmajor != 0;
    p.heavy = a.act == SFCVIT_ACT_GELU || a.dact == SFCVIT_ACT_GELU;
    const bool persistent = fg == SFCVIT_GEMM_AUTO || fg == SFCVIT_GEMM_P8_256 || fg == SFCVIT_GEMM_P8_224 || fg == SFCVIT_GEMM_P8_192;
    if (persistent && (plan_p8(p, a, splits, cus, k) || plan_p8_km(p, a, splits, cus, k))) {
    } else if (persistent && fg != SFCVIT_GEMM_AUTO) {
        REFUSE(SFCVIT_EINVAL, "gemm: shape / options not eligible for the persistent 8-phase kernel");
    } else if (fg == SFCVIT_GEMM_GENERIC || !plan_ring(p, a, splits, k_per_split)) {
        p.family = GemmFamily::GENERIC;
        p.grid = out_tiles * splits;
    }
    if (p.family == GemmFamily::RING || p.family == GemmFamily::GENERIC) {
        p.splits = splits;
        p.k_per_split = k_per_split;
        if (splits > 1) p.reduce_slabs = splits;
    }
    p.actmask_pass = a.actmask && a.act == SFCVIT_ACT_RELU && !(p.mask & P8_BITS);   // the kernel does not write the bits
    p.colsum_pass = a.colsum_out && !(p.mask & P8_CSUM);         // no fused column sums: one pass over the stored C
    return p;
}

namespace {

int check_attn(AttnPlan &p, const sfcvit_attn_args &a, const char *what) {
    const bool bwd = p.bwd;
    if (!a.qkv || !a.out || !a.lse) refuse(p, SFCVIT_EINVAL, "%s: null pointer", what);
    else if (bwd && (!a.dout || !a.dqkv || !a.delta)) refuse(p, SFCVIT_EINVAL, "%s: null pointer", what);
    else if (a.hd != 64 && a.hd != 128 && a.hd != 192 && a.hd != 256)
        refuse(p, SFCVIT_EINVAL, "%s: head dim %d not supported (64, 128, 192, 256)", what, a.hd);
    else if (!(a.dropout_p >= 0.f && a.dropout_p < 1.f)) refuse(p, SFCVIT_EINVAL, "%s: dropout_p=%g out of [0, 1)", what, a.dropout_p);
    else if (a.B <= 0 || a.N <= 0 || a.H <= 0 || a.B > 65535 || a.H > 65535)
        refuse(p, SFCVIT_EINVAL, "%s: B=%d N=%d H=%d", what, a.B, a.N, a.H);
    else if (!aligned(a.qkv, 16) || !aligned(a.out, 16) || (bwd && (!aligned(a.dout, 16) || !aligned(a.dqkv, 16))))
        refuse(p, SFCVIT_EINVAL, "%s: tensors must be 16-byte aligned", what);
    return p.err;
}

// Head dims 128 / 192 / 256: whole sequence in LDS; the default entry points refuse what does not fit.  any_length calls
// stream 64-row blocks instead (attention_wide_stream.hip) where it does not fit, or always with SFCVIT_ATTN_WIDE_STREAM=1.
void plan_wide(AttnPlan &p, const sfcvit_attn_args &a, const Knobs &k, bool any_length) {
    p.family = AttnFamily::WIDE;
    p.inst = a.hd / ATTN_HD;
    p.npad = p.npad2 = (a.N + 31) / 32 * 32;
    p.lds = wide_lds(p.inst, p.npad, p.bwd);                     // bwd: the dK / dV kernel, then the dQ kernel
    p.lds2 = p.bwd ? wide_lds(p.inst, p.npad, false) : 0;
    const bool fits = a.N <= SEQ_MAX_N && p.lds <= size_t(ATTN_LDS_LIMIT);
    if (any_length && (!fits || k.attn_wide_stream)) {
        p.family = AttnFamily::STREAM;
        p.npad = p.npad2 = 0;
        p.lds = stream_lds(p.inst, p.bwd);
        p.lds2 = p.bwd ? stream_lds(p.inst, false) : 0;
        p.grid = (a.N + ATTN_BLK - 1) / ATTN_BLK;
    } else if (!fits) {
        refuse(p, SFCVIT_EINVAL, "attention: head dim %d with N = %d needs %zu KiB of LDS (limit 160); only head dim 64 has a tiled kernel",
               a.hd, a.N, p.lds >> 10);
    }
}

}  // namespace

AttnPlan attn_fwd_plan(const sfcvit_attn_args &a, const Knobs &k, bool any_length) {
    AttnPlan p;
    if (check_attn(p, a, "attention_fwd")) return p;
    p.drop = a.dropout_p > 0.f;
    if (a.hd != ATTN_HD) {
        plan_wide(p, a, k, any_length);
    } else if (a.N <= SEQ_MAX_N) {
        p.family = AttnFamily::SEQ;
        p.npad = (a.N + 15) / 16 * 16;
        p.inst = (a.N + 15) / 16 == 13 ? 13 : 0;
        p.lds = size_t(2 * p.npad * 128);
    } else if (k.attn_long && a.N <= LONG_MAX_N) {
        p.family = AttnFamily::LONG;
        p.npad = (a.N + 31) / 32 * 32;
        p.inst = p.npad == 576 ? 36 : 0;
        p.lds = size_t(2 * p.npad * 128);
    } else {
        p.family = AttnFamily::TILED;
        p.grid = (a.N + ATTN_BLK - 1) / ATTN_BLK;
    }
    return p;
}

AttnPlan attn_bwd_plan(const sfcvit_attn_args &a, int cus, const Knobs &k, bool any_length) {
    AttnPlan p;
    p.bwd = true;
    if (check_attn(p, a, "attention_bwd")) return p;              // (sfcvit_attention_bwd checks colsum_part's size next)
    p.drop = a.dropout_p > 0.f;
    p.colsum = a.colsum_out ? Colsum::PASS : Colsum::NONE;
    if (k.attn_bwd_fused && a.hd == ATTN_HD && a.N <= FUSED_MAX_N) {
        // one pass: dK, dV, dQ, delta and the column sums from a single evaluation of P and dS.  The column sums of dK and dV
        // leave the kernel as 128 floats per item (its key waves hold whole columns).  Those of dQ come from the key waves as
        // well since round 4: sum_q dQ[q, :] = scale sum_k (sum_q dS[q, k]) K[k, :], one add per score in the loop and a
        // 16 x 64 product per wave after it.  (Round 3 took them from the two dQ waves -- per-chunk lane reductions + LDS
        // read-modify-writes on the waves a step waits for, +37 us per launch -- and therefore defaulted to a separate 16-us
        // pass over the Q third of dqkv, which SFCVIT_ATTN_DQSUM=pass still selects: A/B.)
        p.family = AttnFamily::FUSED;
        p.npad = (a.N + 31) / 32 * 32;
        p.inst = (a.N + 15) / 16 == 13 ? 13 : 0;
        p.lds = size_t(p.npad) * FUSED_ROW_BYTES + FUSED_EXTRA + FUSED_POST_BYTES + (p.npad * 128 >= FUSED_CS_BYTES ? 0 : FUSED_CS_BYTES);
        // One workgroup per CU walking the (batch, head) items with the next one staged behind the current (kernel header);
        // SFCVIT_ATTN_BWD_PERSIST=0: one workgroup per item, i.e. the kernel of rounds 2-3 (A/B).
        const int items = a.B * a.H;
        p.grid = cus > 0 && k.attn_bwd_persist ? (items < cus ? items : cus) : items;
        p.queue = k.attn_bwd_queue && p.grid < items;
        // Start-up stagger (attention_common.h): every workgroup opens with a 117 KiB load burst and they all take the same
        // time, so launched together they stay in lockstep.  Two slots 4.5 us apart: 270.8 -> 257.1 us at ViT-B / 256 with one
        // workgroup per item (3 or 4 slots, 2-8 us: 255.6-258.6).  The persistent form (round 4) pays the burst once per 12
        // items and its workgroups drift apart on their own: the stagger costs it 5 us (227.6 vs 222.7 us,
        // profiles/r4/attention_bench_r4.txt), so it is on for one-workgroup-per-item launches only.
        const int slots = k.attn_stagger_slots > 0 ? k.attn_stagger_slots : p.grid < items ? 1 : 2;
        p.round = 256;
        p.per = (p.round + slots - 1) / slots;
        p.ticks = k.attn_stagger_ticks;
        p.nt = k.attn_nt & 1;
        p.dq_sums = k.attn_dq_in_kernel;
        if (a.colsum_out) p.colsum = k.attn_dq_in_kernel ? Colsum::PARTIALS : Colsum::PARTIALS_QPASS;
    } else if (k.attn_long && a.hd == ATTN_HD && a.N > SEQ_MAX_N && a.N <= LONG_MAX_N) {
        // sequence-resident kernels: delta comes out of their dQ kernel (first), the column sums too
        p.family = AttnFamily::LONG;
        p.npad = p.npad2 = (a.N + 31) / 32 * 32;
        p.lds = size_t(2 * p.npad * 128);
        p.lds2 = size_t(2 * p.npad * 128 + 3 * p.npad * 4);
        if (a.colsum_out) p.colsum = Colsum::PARTIALS;
    } else if (a.hd != ATTN_HD) {                                   // these need the delta pass first
        plan_wide(p, a, k, any_length);
    } else if (a.N <= SEQ_MAX_N) {
        p.family = AttnFamily::SEQ;
        p.inst = (a.N + 15) / 16 == 13 ? 13 : 0;
        p.npad = (a.N + 31) / 32 * 32;                           // dK / dV kernel
        p.npad2 = (a.N + 15) / 16 * 16;                          // dQ kernel
        p.lds = size_t(2 * p.npad * 128 + 3 * p.npad * 4);
        p.lds2 = size_t(2 * p.npad2 * 128);
    } else {
        p.family = AttnFamily::TILED;
        p.grid = (a.N + ATTN_BLK - 1) / ATTN_BLK;
    }
    return p;
}

void kernel_name(const GemmPlan &p, char *buf, size_t n) {
    const char *tf[2] = {"false", "true"};
    switch (p.family) {
    case GemmFamily::P8: snprintf(buf, n, "gemm8p_kernel<%d, %d, %s>", p.ni, p.mask, tf[p.p2]); break;
    case GemmFamily::P8_KM: snprintf(buf, n, "gemm8p_km_kernel<%s>", tf[p.p2]); break;
    case GemmFamily::RING: snprintf(buf, n, "gemm256_kernel<%s, %s, %d, %s>", tf[p.a_km], tf[p.b_km], p.bn, tf[p.heavy]); break;
    case GemmFamily::GENERIC: snprintf(buf, n, "gemm_kernel<%s, %s, %s>", tf[p.a_km], tf[p.b_km], tf[p.heavy]); break;
    }
}

void kernel_name(const AttnPlan &p, char *buf, size_t n) {
    const char *drop = p.drop ? "true" : "false";
    switch (p.family) {
    case AttnFamily::WIDE: snprintf(buf, n, p.bwd ? "attn_wide_bwd_kv_kernel<%d>" : "attn_wide_fwd_kernel<%d>", p.inst); break;
    case AttnFamily::SEQ:
        if (p.bwd) snprintf(buf, n, "attn_seq_bwd_kv_kernel<%d>", p.inst);
        else snprintf(buf, n, "attn_seq_fwd_kernel<%d, %s>", p.inst, drop);
        break;
    case AttnFamily::LONG:
        if (p.bwd) snprintf(buf, n, "attn_long_bwd_kv_kernel");
        else snprintf(buf, n, "attn_long_fwd_kernel<%d>", p.inst);
        break;
    case AttnFamily::TILED: snprintf(buf, n, p.bwd ? "attn_bwd_kv_kernel" : "attn_fwd_kernel"); break;
    case AttnFamily::FUSED: snprintf(buf, n, "attn_seq_bwd_fused_kernel<%d, %s>", p.inst, drop); break;
    case AttnFamily::STREAM:
        snprintf(buf, n, p.bwd ? "attn_wide_stream_bwd_kv_kernel<%d>" : "attn_wide_stream_fwd_kernel<%d>", p.inst);
        break;
    }
}

}  // namespace sfcvit
