// api_chain.hip -- the chain dispatch: which kernels a stage mask runs for the context's settings and which scratch they
// take, decided once per call (plan_chain -> ChainPlan), what carries the plan out (run_native: the frame kernel's variant or
// the unfused sequence; run_chain: + TII, Resampler, MemlessPoly, FormatConverter), and the chain's entry points.
#include "dabgpu_ctx.h"

using namespace dabgpu;
using namespace dabgpu_api;

namespace dabgpu_api {
int auto_chunks(const dabgpu_ctx *c, size_t n_frames)
{
    if (c->chunks_cfg > 0) return c->chunks_cfg;
    // One workgroup per frame once the batch alone fills the chip (1024 workgroups: four per CU); below that frames are
    // split into runs of symbols so that the launch still has about 1024 of them.  Every run pays a prologue (the
    // differential state up to its first symbol: a bit-sliced sum over the blocks before it, a few microseconds whatever
    // the depth) and, with FIR, one look-ahead transform.  Measured optimum, Mode I (tools/sweep_chunks.py, round 3):
    // 1024 / B runs down to B = 32, two symbols per run for 14 ... 31 frames, single symbols below (latency, not
    // efficiency, counts there: 10 us per Mode-I frame).
    // With the call rotating over L lanes (section 4.5 of DESIGN.md), L launches are in flight and the chip is filled by
    // FEWER, LONGER runs per launch -- and every run saved is a prologue and a look-ahead transform saved: measured optimum
    // with three lanes (tools/experiments/exp_r05.py chunks, profiles/r05_exp_chunks.jsonl) 26 runs per frame at 16 frames (416 workgroups;
    // +10 % over 624), 6 ... 8 at 64 (+14 % over 1024), 2 at 256 (+4 %): about 1280 / L workgroups per launch.
    const int nsym = c->g.nb_symbols + 1;
    const size_t n = n_frames;
    const size_t target = c->call_lanes > 1 ? std::max<size_t>(256, 1280 / (size_t)c->call_lanes) : 1024;
    const int want = std::max(1, std::min(n >= target ? 1 : (int)((target + n - 1) / n), nsym));
    // no empty runs: the callers give every run ceil(nsym / chunks) symbols, so ask for exactly as many runs as that
    // run length needs (74 wanted -> 2 symbols per run -> 39 runs, not 74 workgroups of which 35 return after the prologue)
    const int per_run = (nsym + want - 1) / want;
    return (nsym + per_run - 1) / per_run;
}

// Symbols per run of a frame cut into `chunks` runs.  A run of a chain with FIRFilter or a windowed guard interval transforms
// one symbol MORE than it stores (the look-ahead symbol its last boundary needs) -- except the frame's last run, which ends
// with the frame.  So the last run takes one symbol more than the others where that evens them out: 77 symbols in four runs
// are 19 + 1, 19 + 1, 19 + 1, 20 transforms, not 20 + 1, 20 + 1, 20 + 1, 17 (the kernel gives the last run whatever is left).
int run_symbols(int nsym, int chunks, bool lookahead)
{
    return std::max(1, (nsym - (lookahead ? 1 : 0) + chunks - 1) / chunks);
}

bool is_pow2(size_t x) { return x && !(x & (x - 1)); }

// ratios with a dedicated kernel (integer 2 and 4: packed dual transforms, fused predistorter)
bool resampler_fast_ratio(const dabgpu_ctx *c)
{
    return c->rs_nout % c->rs_nin == 0 && (c->rs_nout / c->rs_nin == 2 || c->rs_nout / c->rs_nin == 4);
}

// the polynomial predistorter as an epilogue of the x2 / x4 resampler's store (LUT mode is a kernel of its own)
bool poly_in_resampler(const dabgpu_ctx *c, unsigned mask)
{
    return (mask & DABGPU_STAGE_RESAMPLE) && (mask & DABGPU_STAGE_POLY) && !c->cur.poly_is_lut && resampler_fast_ratio(c);
}

// Ratios the kernels cover: L / M (reduced) with M a power of two up to the FFT size N of the transmission mode,
// any L -- up- and down-sampling.  Then nin = 2 N is a power of two and the nout = (nin / M) L point transform
// factors into L branches of nin / M points.  Every other ratio is one the reference itself cannot run on whole
// transmission frames: with M = 2^a 5^b, b > 0 (the input rate is 2 048 000 = 2^14 5^3), half its FFT size does
// not divide the frame length, and its hop loop (src/Resampler.cpp:142) runs past the input buffer; with M > N
// its `factor` is 1 or 0 (src/Resampler.cpp:69-75).
const char *resampler_ratio_error(int N, size_t in_rate, size_t out_rate)
{
    if (!in_rate || !out_rate) return "Resampler: invalid rate";
    if (in_rate == out_rate) return nullptr;
    size_t a = in_rate, b = out_rate;
    while (b) { size_t t = a % b; a = b; b = t; }
    const size_t L = out_rate / a, M = in_rate / a;
    if (!is_pow2(M) || M > (size_t)N)
        return "Resampler: only ratios L/M with M a power of two up to the FFT size are supported "
               "(the reference's hop size does not divide a transmission frame for any other)";
    if ((2 * (size_t)N / M) * L > ((size_t)1 << 20)) return "Resampler: output FFT size beyond 2^20";
    return nullptr;
}

const char *resampler_error(const dabgpu_ctx *c)
{
    const char *e = resampler_ratio_error(c->g.N, c->cur.rs_in, c->cur.rs_out);
    if (e) return e;
    if ((size_t)c->rs_nin != 2 * (size_t)c->g.N || (size_t)c->rs_nout != (size_t)c->rs_nin / c->rs_M * c->rs_L)
        return "Resampler: inconsistent geometry";
    return nullptr;
}

int check_resampler(dabgpu_ctx *c)
{
    const char *e = resampler_error(c);
    return e ? fail(c, DABGPU_E_INVALID, e) : DABGPU_OK;
}

// stream of `total` samples at d_in -> resampled at d_out (stateful)
int run_resampler(dabgpu_ctx *c, const float2 *d_in, size_t total, float2 *d_out, hipStream_t s,
                  bool fuse_poly, unsigned long long *s16_clipped)
{
    int rc = check_resampler(c);
    if (rc) return rc;
    const size_t hin = (size_t)c->rs_nin / 2;
    if (total % hin) return fail(c, DABGPU_E_INVALID, "Resampler::process input size not valid!");
    const size_t nhops = total / hin;
    if (nhops == 0) return DABGPU_OK;     // (nothing in, nothing out, the state -- halo buffers included -- as it was)
    ResamplerArgs a{};
    a.nin = c->rs_nin; a.nout = c->rs_nout; a.factor = c->rs_factor;
    a.window = (const float *)c->d_rs_window.p;
    a.tw_in = (const float2 *)c->d_rs_tw_in.p;
    a.tw_out = (const float2 *)c->d_rs_tw_out.p;
    float2 *halo = (float2 *)c->d_rs_halo.p + (size_t)c->rs_halo_cur * (size_t)c->rs_nin;
    float2 *halo_next = (float2 *)c->d_rs_halo.p + (size_t)(c->rs_halo_cur ^ 1) * (size_t)c->rs_nin;
    a.in = d_in; a.halo = halo;
    a.out = d_out; a.nhops = nhops;
    a.poly = (fuse_poly && resampler_fast_ratio(c)) ? (const float *)c->d_coef.p : nullptr;
    a.clipped = s16_clipped;
    a.L = (int)c->rs_L;
    a.M = (int)c->rs_M;
    a.tw_s = (const float2 *)c->d_rs_tw_s.p;
    a.tw_l = (const float2 *)c->d_rs_tw_l.p;
    a.run_hops = c->rs_run_hops;
    // new halo = last two hops of the concatenation [halo | in]: the x2 / x4 kernel of Mode I writes it itself, into the
    // other buffer (launches of one stream are in order: the next call reads what this one wrote)
    if (resampler_writes_halo(a)) {
        a.halo_out = halo_next;
        HIPCHK(c, launch_resampler(a, s));
        resampler_last_launch(&c->rs_last_hops, &c->rs_last_grid);
        c->rs_halo_cur ^= 1;
        return DABGPU_OK;
    }
    HIPCHK(c, launch_resampler(a, s));
    resampler_last_launch(&c->rs_last_hops, &c->rs_last_grid);
    if (nhops >= 2) {
        HIPCHK(c, hipMemcpyAsync(halo, d_in + (nhops - 2) * hin, 2 * hin * sizeof(float2),
                                 hipMemcpyDeviceToDevice, s));
    } else {
        HIPCHK(c, hipMemcpyAsync(halo, halo + hin, hin * sizeof(float2), hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(halo + hin, d_in, hin * sizeof(float2), hipMemcpyDeviceToDevice, s));
    }
    return DABGPU_OK;
}

int run_poly(dabgpu_ctx *c, const float2 *d_in, size_t n, float2 *d_out, hipStream_t s)
{
    const float *coef = (const float *)c->d_coef.p;
    if (c->cur.poly_is_lut)
        HIPCHK(c, launch_lut(d_in, n, c->cur.lut_scale, coef + 16, d_out, s));
    else
        HIPCHK(c, launch_poly(d_in, n, coef, coef + 8, d_out, s));
    return DABGPU_OK;
}

size_t bytes_per_sample(int fmt) { return fmt ? dabgpu_format_size(fmt) : sizeof(float2); }

// The one place a stage mask is normalised and a frame's output is sized: the Resampler at equal rates is not in the chain
// (src/DabModulator.cpp:336-340), and behind it a frame has L / M (reduced) times its native-rate samples.
unsigned normalised_mask(const Settings &st, unsigned mask)
{
    return st.rs_in == st.rs_out ? mask & ~(unsigned)DABGPU_STAGE_RESAMPLE : mask;
}

size_t out_samples_per_frame(const Geometry &g, const Settings &st, unsigned mask)
{
    size_t n = (mask & DABGPU_STAGE_NOGUARD) ? (size_t)(g.nb_symbols + 1) * (size_t)g.N : tf_samples(g);
    if (!(normalised_mask(st, mask) & DABGPU_STAGE_RESAMPLE)) return n;
    size_t a = st.rs_in, b = st.rs_out;
    while (b) { size_t t = a % b; a = b; b = t; }
    return n * (st.rs_out / a) / (st.rs_in / a);
}

// Which kernels a chain call runs and which per-lane scratch it reserves, decided ONCE: run_chain / run_native /
// ensure_tii_segment do what the plan says, and the lane choice (api_lanes.hip) reads its scratch total.  Reads the applied
// settings (c->cur) and the context facts the decision depends on (eq_ok, use_eq, chunks_cfg, call_lanes, handover_frames,
// the resampler's geometry); calls nothing in HIP, reserves nothing, allocates nothing.  The tf_has_* predicates of
// tf_launch.hip are the single source of "this variant exists in this build", and this function is their only caller
// outside the launchers.
// from_bits: the input is coded bits, else carriers.  keep_stats: the CFR statistics are the caller's to read (a chain call);
// false for the chain's internal runs (the TII segment, the pieces of the hand-over).
// cic: carriers first -- the front kernel (coded bits -> equalised carriers, or cic_kernel on the caller's carriers) into
// d_car, then exactly the plan this function gives for the same mask from carriers.
ChainPlan plan_chain(const dabgpu_ctx *c, bool from_bits, size_t n_frames, unsigned mask, bool apply_format, bool keep_stats,
                     bool cic)
{
    const Settings &st = c->cur;
    const Geometry &g = c->g;
    if (cic) {
        ChainPlan p = plan_chain(c, /*from_bits=*/false, n_frames, mask, apply_format, keep_stats, false);
        p.front = from_bits ? ChainPlan::FRONT_BITS : ChainPlan::FRONT_CIC;
        if (!p.error && n_frames) {
            p.scratch.d_car = n_frames * (size_t)(g.nb_symbols + 1) * (size_t)g.K * sizeof(float2);
            p.scratch_bytes += p.scratch.d_car;
        }
        return p;
    }
    ChainPlan p;
    p.from_bits = from_bits;
    p.keep_stats = keep_stats;
    p.n_frames = n_frames;
    p.mask = mask = normalised_mask(st, mask);
    const bool noguard = mask & DABGPU_STAGE_NOGUARD, fir = mask & DABGPU_STAGE_FIR, gain = mask & DABGPU_STAGE_GAIN,
               resample = mask & DABGPU_STAGE_RESAMPLE, poly = mask & DABGPU_STAGE_POLY;
    // FormatConverter as the last step of the chain (src/DabModulator.cpp:395-419): the stage-level entry points
    // that borrow the chain (OfdmGenerator, the TII segment) stay complexf
    p.fmt = apply_format ? st.out_format : 0;
    p.per = out_samples_per_frame(g, st, mask);
    p.native = noguard ? p.per : tf_samples(g);
    p.out_bytes = n_frames * p.per * bytes_per_sample(p.fmt);
    if (noguard && (fir || resample || poly)) p.error = "NOGUARD cannot be combined with FIR/RESAMPLE/POLY";
    else if (fir && st.taps.empty()) p.error = "FIRFilter: no taps loaded";
    else if (resample) p.error = resampler_error(c);
    if (p.error || n_frames == 0) return p;

    const int nsym = g.nb_symbols + 1, ntaps = (int)st.taps.size(), cp = g.sym_size - g.N;
    const size_t nsymN = (size_t)nsym * (size_t)g.N;
    const bool post = resample || poly;
    const bool fast_ratio = resample && resampler_fast_ratio(c);
    const bool fir_fits = ntaps - 1 <= cp && ntaps <= tf_max_fused_taps();
    // one fused kernel, unless the guard interval is windowed or the filter does not fit it
    // (then: IFFT[+CFR][+gain] -> guard kernel -> FIR kernel)
    // (CFR has fused variants with the whole epilogue -- guard + FIR --, with none of it, and, from coded bits, with the
    // guard interval alone)
    const bool windowed = (st.overlap > 0 || (fir && !fir_fits) || (st.cfr_enable && !fir && !from_bits)) && !noguard;
    if (windowed && st.overlap > (size_t)cp) {
        p.error = "window overlap larger than the guard interval";
        return p;
    }
    p.tii = from_bits && st.tii_enable;
    // gain mode var by the reference's recurrence (dabgpu_set_gain_rounding): the chain call is split at GainControl
    const bool replay = st.gain_reference_rounding && st.gain_mode == DABGPU_GAIN_VAR && gain;
    // Tap count the frame kernel is given.  A filter of fewer than 45 taps runs as a 45-tap filter whose last taps are zero
    // (out[n] = sum_j taps[j] in[n + j]: zero taps add nothing; the device table is zero padded) -- the kernels with the
    // compile-time tap count, the equalised-boundary variant among them, then serve every filter up to the default length.
    const int fused_ntaps = (ntaps >= 1 && ntaps < 45) ? 45 : ntaps;

    // what the predicates look at
    TfArgs a{};
    a.g = g;
    a.t.eq_g = c->eq_ok ? (const float *)c->d_eqg.p : nullptr;
    a.gain.mode = st.gain_mode;
    a.ntaps = ntaps;
    a.overlap = (int)st.overlap;
    unsigned flags = (from_bits ? TF_FROM_BITS : 0) | (gain && !replay ? TF_GAIN : 0) | (st.cfr_enable ? TF_CFR : 0);
    const unsigned ofmt = (from_bits && !post && !replay) ? tf_ofmt_flag(p.fmt) : 0;   // (the frame kernel is the chain's last)
    p.chunks_per_frame = auto_chunks(c, n_frames);
    bool lookahead = false;
    p.form = ChainPlan::UNFUSED;
    if (replay) {
        // OfdmGenerator (+ CFR) alone, then the reference's recurrence on the unscaled symbols (src/GainControl.cpp:118-155),
        // then guard interval / FIRFilter as kernels of their own, which scale the symbols as they read them
        p.form = ChainPlan::GAIN_REPLAY;
        p.scratch.d_gains = n_frames * (size_t)nsym * sizeof(float);
    } else if (!windowed) {
        p.form = ChainPlan::ONE_KERNEL;
        flags |= (noguard ? 0 : TF_GUARD) | (fir ? TF_FIR : 0);
        if (!st.cfr_enable) a.ntaps = fused_ntaps;      // (the CFR variants loop over the run-time tap count)
        // cfg 3 chain: the filtered transform alone with equalised boundaries (dabgpu_set_fir_boundary_mode(ctx, 1): the
        // packed dual transform)
        if (c->use_eq && tf_has_eq(a, flags)) flags |= TF_EQ;
        lookahead = fir;
    } else if (tf_has_window(a, flags | TF_GUARD | (fir ? TF_FIR : 0))) {
        // OFDM windowing on the coded-bits chain, with or without FIRFilter: the frame kernel windows the guard interval
        // itself (and filters across the seams)
        p.form = ChainPlan::ONE_KERNEL;
        flags |= TF_GUARD | TF_WINDOW | (fir ? TF_FIR : 0);
        if (c->use_eq && fir && !st.cfr_enable) {
            // narrow overlaps on the cfg 3 chain: the equalised-boundary variant with the seam inside its boundary outputs
            // (the filter run at the default length, as without windowing)
            a.ntaps = fused_ntaps;
            if (tf_has_eq(a, flags)) flags |= TF_EQ;
            else a.ntaps = ntaps;
        }
        lookahead = true;
    }
    p.ntaps = a.ntaps;
    p.syms_per_chunk = a.syms_per_chunk = run_symbols(nsym, p.chunks_per_frame, lookahead);
    const bool one_kernel = p.form == ChainPlan::ONE_KERNEL;
    // TII is added to the native-rate complexf stream afterwards unless the frame kernel adds it itself
    p.tii_inside = p.tii && one_kernel && tf_has_tii(a, flags);
    // An integer format leaves the LAST kernel of the chain directly where that kernel has a variant for it (every other
    // combination converts afterwards, through d_fmt): the frame kernel -- asked of the kernels' own predicates, the ones
    // their launchers test, so that the separate convert kernel is taken whenever a variant does not exist in this build.
    // u8 / s8: its equalised-boundary and no-FIRFilter variants; s16: those, the pruned dual transform, CFR.  Of the forms
    // with a windowed guard interval: the equalised-boundary one (every format, TII inside) and the chain without
    // FIRFilter (s16, no TII).
    if (ofmt && one_kernel && (!p.tii || p.tii_inside) && tf_has_fmt(a, flags | ofmt)) {
        p.fuse_native = true;
        flags |= ofmt;
    }
    p.tf_flags = flags;
    // ... or the x2 / x4 resampler (s16; with the polynomial predistorter inside its store, or none)
    p.fuse_poly = poly_in_resampler(c, mask);
    if (p.fmt == DABGPU_FMT_S16 && from_bits && fast_ratio && (!poly || !st.poly_is_lut)) {
        ResamplerArgs ra{};
        ra.nin = c->rs_nin;
        ra.nout = c->rs_nout;
        p.fuse_post = resampler_has_s16(ra);
    }

    // ---- the per-lane scratch the call reserves
    if (!one_kernel && !noguard) p.scratch.d_b = n_frames * nsymN * sizeof(float2);        // the symbols before the guard kernel
    if (p.fmt && !p.fuse_native && !p.fuse_post) p.scratch.d_fmt = n_frames * p.per * sizeof(float2);
    if (st.cfr_enable) {
        // crest-factor reduction inside OfdmGenerator (f-3): statistics per frame
        p.scratch.cfr_counts = n_frames * 2 * sizeof(unsigned);
        p.scratch.cfr_mer = n_frames * 2 * sizeof(double);
        p.scratch.cfr_papr = n_frames * (size_t)nsym * 4 * sizeof(double);
        if (!keep_stats) p.scratch.cfr_tmp = p.scratch.cfr_counts + p.scratch.cfr_mer + p.scratch.cfr_papr + 16;
    }
    // The hand-over FIRFilter -> Resampler in cache-sized pieces (dabgpu_set_handover_frames): x2 / x4 with the predistorter
    // inside the resampler's store or absent; CFR (per-frame statistics) and TII (per-frame gain, frame parity) keep the
    // one-piece path.
    const size_t piece = (size_t)c->handover_frames & ~(size_t)1;
    if (fast_ratio && (p.fuse_poly || !poly) && !st.cfr_enable && !p.tii && piece >= 2 && n_frames > piece) {
        p.piece = piece;
        const size_t d_fmt = p.scratch.d_fmt;
        // (what the native-rate part of one piece reserves, with a plan of its own; the two-piece ring)
        p.scratch = plan_chain(c, from_bits, piece, mask & ~(unsigned)(DABGPU_STAGE_RESAMPLE | DABGPU_STAGE_POLY), false, false)
                        .scratch;
        p.scratch.d_a = 2 * piece * p.native * sizeof(float2);
        p.scratch.d_fmt = d_fmt;
    } else {
        if (post) p.scratch.d_a = n_frames * p.native * sizeof(float2);     // the native-rate stream
        if (resample && poly && !p.fuse_poly)                               // the resampled stream in front of the predistorter
            p.scratch.d_b = std::max(p.scratch.d_b, n_frames * p.per * sizeof(float2));
        if (p.tii) {
            if (gain) p.scratch.d_gain1 = n_frames * sizeof(float);
            // (the one-frame run from carriers that builds the cached TII segment, on this call's lane)
            const ChainPlan::Scratch seg = plan_chain(c, false, 1, mask & (DABGPU_STAGE_FIR | DABGPU_STAGE_NOGUARD), false, false).scratch;
            p.scratch.d_b = std::max(p.scratch.d_b, seg.d_b);
            p.scratch.cfr_tmp = std::max(p.scratch.cfr_tmp, seg.cfr_tmp);
        }
    }
    const ChainPlan::Scratch &sc = p.scratch;
    p.scratch_bytes = sc.d_a + sc.d_b + sc.d_fmt + sc.d_gains + sc.d_gain1 + sc.cfr_tmp +
                      (keep_stats ? sc.cfr_counts + sc.cfr_mer + sc.cfr_papr : 0);
    return p;
}

// The native-rate part of the chain (everything up to and including FIRFilter) as the plan has it, into native_out
// (p.native samples per frame).  TII: the frame kernel adds the cached segment where the plan says so (else run_chain does).
int run_native(dabgpu_ctx *c, const ChainPlan &p, const void *d_in, float2 *native_out, hipStream_t s)
{
    const int nsym = c->g.nb_symbols + 1;
    const size_t n_frames = p.n_frames;
    const bool noguard = p.mask & DABGPU_STAGE_NOGUARD;
    float *gain1 = p.scratch.d_gain1 ? (float *)c->d_gain1.p : nullptr;
    TfArgs a{};
    a.clipped = p.fuse_native ? (unsigned long long *)c->d_clip.p : nullptr;   // (the frame kernel stores the integers itself)
#ifdef DABGPU_PHASE_TIMING
    a.phase_cycles = (unsigned long long *)c->d_phase.p;
#endif
    a.g = c->g;
    a.t = tables_of(c);
    a.gain = gain_of(c);
    a.ntaps = p.ntaps;
    a.n_frames = (int)n_frames;
    a.bits = p.from_bits ? (const uint8_t *)d_in : nullptr;
    a.carriers = p.from_bits ? nullptr : (const float2 *)d_in;
    a.gain1 = (p.from_bits && p.form != ChainPlan::GAIN_REPLAY) ? gain1 : nullptr;
    a.overlap = (int)c->cur.overlap;
    a.chunks_per_frame = p.chunks_per_frame;
    a.syms_per_chunk = p.syms_per_chunk;
    if (p.tf_flags & TF_CFR) {
        // crest-factor reduction inside OfdmGenerator (f-3): statistics per frame, zeroed per call
        a.cfr_clip = c->cur.cfr_clip;
        a.cfr_errclip = c->cur.cfr_errclip;
        if (p.keep_stats) {
            HIPCHK(c, c->d_cfr_counts.reserve(p.scratch.cfr_counts));
            HIPCHK(c, c->d_cfr_mer.reserve(p.scratch.cfr_mer));
            HIPCHK(c, c->d_cfr_papr.reserve(p.scratch.cfr_papr));
            a.cfr_counts = (unsigned *)c->d_cfr_counts.p;
            a.cfr_mer = (double *)c->d_cfr_mer.p;
            a.cfr_papr = (double *)c->d_cfr_papr.p;
            a.cfr_mer_base = c->cfr_mer_index + 1;                       // src/OfdmGenerator.cpp:198
            c->cfr_last_base = a.cfr_mer_base;
            c->cfr_last_frames = n_frames;
            c->cfr_last_stream = s;
            c->cfr_mer_index = (int)((c->cfr_mer_index + n_frames) % (size_t)nsym);
        } else {
            HIPCHK(c, c->d_cfr_tmp.reserve(p.scratch.cfr_tmp));
            a.cfr_mer = (double *)c->d_cfr_tmp.p;
            a.cfr_papr = a.cfr_mer + n_frames * 2;
            a.cfr_counts = (unsigned *)(a.cfr_papr + n_frames * (size_t)nsym * 4);
            a.cfr_mer_base = 0;
        }
        HIPCHK(c, hipMemsetAsync(a.cfr_counts, 0, p.scratch.cfr_counts, s));
        HIPCHK(c, hipMemsetAsync(a.cfr_mer, 0, p.scratch.cfr_mer, s));
        HIPCHK(c, hipMemsetAsync(a.cfr_papr, 0, p.scratch.cfr_papr, s));
    }
    // the frame kernel writes the native-rate stream itself, or the symbols ((nb_symbols + 1) x N per frame) for the guard kernel
    const bool one_kernel = p.form == ChainPlan::ONE_KERNEL;
    float2 *x0 = native_out;
    if (!one_kernel && !noguard) {
        HIPCHK(c, c->d_b.reserve(p.scratch.d_b));
        x0 = (float2 *)c->d_b.p;
    }
    a.out = x0;
    a.out_stride = x0 == native_out ? p.native : (size_t)nsym * (size_t)c->g.N;
    if (p.tii_inside) {
        a.tii_seg = (const float2 *)c->d_tii_frame.p;
        a.tii_insert0 = c->tii_insert ? 1 : 0;
    }
    HIPCHK(c, launch_tf(a, p.tf_flags, s));
    if (one_kernel) return DABGPU_OK;

    const float *gains = nullptr;
    if (p.form == ChainPlan::GAIN_REPLAY) {
        // (the multipliers are applied by the guard kernel as it gathers the symbols; a chain that stops here scales in place)
        HIPCHK(c, c->d_gains.reserve(p.scratch.d_gains));
        gains = (const float *)c->d_gains.p;
        HIPCHK(c, launch_gain_replay(x0, n_frames, nsym, c->g.N, a.gain, (float *)c->d_gains.p, p.from_bits ? gain1 : nullptr,
                                     noguard, s));
        if (noguard) return DABGPU_OK;
    }
    if (p.mask & DABGPU_STAGE_FIR)
        HIPCHK(c, launch_guard_fir(x0, n_frames, c->g, (int)c->cur.overlap, (const float *)c->d_window.p, c->cur.taps.data(),
                                   (int)c->cur.taps.size(), native_out, s, gains));
    else if (c->cur.overlap > 0)
        HIPCHK(c, launch_guard_window(x0, n_frames, c->g, (int)c->cur.overlap, (const float *)c->d_window.p, native_out, s, gains));
    else
        HIPCHK(c, launch_guard_copy(x0, n_frames, c->g, native_out, s, gains));
    return DABGPU_OK;
}

// TII A_{c,p} in the reference's index convention (src/TII.cpp:247-337)
int tii_carrier_set(int mode, int comb, int pattern, std::vector<uint8_t> &acp)
{
    const int K = mode == 1 ? 1536 : 384;
    acp.assign((size_t)K, 0);
    // the 70 patterns are the 8-bit words of weight 4 in increasing order, leftmost bit = b 0 (:34-104)
    int word = 0;
    for (int w = 0, idx = 0; w < 256; ++w)
        if (__builtin_popcount((unsigned)w) == 4 && idx++ == pattern) word = w;
    auto enable = [&](int k) {
        const int ix = K / 2 + k + (k >= 0 ? -1 : 0);
        if (ix < 0 || ix + 1 >= K) return false;
        acp[(size_t)ix] = 1;
        return true;
    };
    bool ok = true;
    for (int b = 0; b < 8; ++b) {
        if (!((word >> (7 - b)) & 1)) continue;
        if (mode == 1) {
            for (int base : {-768, -384, 1, 385}) ok = enable(base + 2 * comb + 48 * b) && ok;
        } else {
            ok = enable((b < 4 ? -192 : -191) + 2 * comb + 48 * b) && ok;
        }
    }
    return ok ? DABGPU_OK : DABGPU_E_INVALID;
}

// (Re)build the stream contribution of one TII null symbol at unit gain for this stage mask:
// TII symbol -> IFFT -> guard interval (-> FIR) of a frame whose other symbols are blank.
int ensure_tii_segment(dabgpu_ctx *c, unsigned mask, hipStream_t s)
{
    const unsigned key = mask & (DABGPU_STAGE_FIR | DABGPU_STAGE_NOGUARD);
    if (c->tii_seg_epoch != 0 && c->tii_seg_mask == key) return DABGPU_OK;
    // the segment is built from CARRIERS, by a one-frame run with a plan of its own (CFR with the guard interval alone is
    // fused from coded bits only: from carriers that combination takes the unfused IFFT + CFR -> guard kernels)
    const ChainPlan seg = plan_chain(c, false, 1, key, false, false);
    if (seg.error) return fail(c, DABGPU_E_INVALID, seg.error);
    const size_t K = (size_t)c->g.K, car_bytes = (size_t)(c->g.nb_symbols + 1) * K * sizeof(float2);
    std::vector<uint8_t> acp;
    if (tii_carrier_set(c->g.mode, c->cur.tii_comb, c->cur.tii_pattern, acp))
        return fail(c, DABGPU_E_INVALID, "TII::enable_carrier invalid k!");
    // d_acp / d_tii_car / d_tii_frame are shared by the lanes: batches still in flight on ANOTHER lane read the old
    // segment (in-kernel, or launch_tii_add) -- they finish before it is overwritten.  Once per TII / CFR setting or mask.
    {
        const int rc_drain = drain_lanes(c);
        if (rc_drain) return rc_drain;
    }
    HIPCHK(c, upload(c->d_acp, acp, s));
    HIPCHK(c, c->d_tii_car.reserve(car_bytes + K * sizeof(float2)));
    HIPCHK(c, c->d_tii_frame.reserve(seg.native * sizeof(float2)));
    HIPCHK(c, hipMemsetAsync(c->d_tii_car.p, 0, car_bytes, s));
    float2 *phase = (float2 *)((char *)c->d_tii_car.p + car_bytes);
    HIPCHK(c, launch_phase_reference((const uint8_t *)c->d_phq.p, c->g.K, phase, s));
    HIPCHK(c, launch_tii(phase, (const uint8_t *)c->d_acp.p, c->g.K, c->cur.tii_old_variant ? 1 : 0, 1,
                         (float2 *)c->d_tii_car.p, s));
    const int rc = run_native(c, seg, c->d_tii_car.p, (float2 *)c->d_tii_frame.p, s);
    if (rc) return rc;
    // the response of the null symbol: its own segment plus whatever a windowed guard interval spills
    // into the next one (zeros beyond; adding them is harmless)
    const size_t ext = (mask & DABGPU_STAGE_NOGUARD) ? (size_t)c->g.N
                                                     : (size_t)c->g.null_size + 2 * c->cur.overlap + 8;
    c->tii_seg_len = (int)std::min(seg.native, ext);
    HIPCHK(c, hipStreamSynchronize(s));   // (once per setting: the segment is read by whichever lane runs the next call)
    c->tii_seg_epoch = 1;
    c->tii_seg_mask = key;
    return DABGPU_OK;
}

// The native-rate stream of a call with the TII null symbol in it (src/TII.cpp:226-242: every other frame, from
// c->tii_insert on): run_native, with the cached segment built first and added afterwards where the frame kernel does not
// add it itself.  What run_chain runs in front of the tail -- and what dabgpu_chain_seed runs on the lead-in frame.
int run_native_tii(dabgpu_ctx *c, const ChainPlan &p, const void *d_in, float2 *native_out, hipStream_t s)
{
    int rc;
    if (p.tii) {
        if ((rc = ensure_tii_segment(c, p.mask, s))) return rc;
        HIPCHK(c, c->d_gain1.reserve(p.scratch.d_gain1));
    }
    if ((rc = run_native(c, p, d_in, native_out, s))) return rc;
    if (p.tii && !p.tii_inside)
        HIPCHK(c, launch_tii_add(native_out, p.native, (const float2 *)c->d_tii_frame.p, c->tii_seg_len,
                                 p.scratch.d_gain1 ? (const float *)c->d_gain1.p : nullptr, c->tii_insert ? 1 : 0, p.n_frames, s));
    return DABGPU_OK;
}

// The TII carrier set the carriers kernel reads, for the settings in force.  One buffer for all lanes: kernels in flight on
// another lane read the old set -- they finish before it is rewritten (as ensure_tii_segment does with its tables).
int ensure_carrier_acp(dabgpu_ctx *c, hipStream_t s)
{
    if (c->car_acp_comb == c->cur.tii_comb && c->car_acp_pattern == c->cur.tii_pattern) return DABGPU_OK;
    std::vector<uint8_t> acp;
    if (tii_carrier_set(c->g.mode, c->cur.tii_comb, c->cur.tii_pattern, acp))
        return fail(c, DABGPU_E_INVALID, "TII::enable_carrier invalid k!");
    const int rc = drain_lanes(c);
    if (rc) return rc;
    c->car_acp_comb = c->car_acp_pattern = -1;
    HIPCHK(c, upload(c->d_car_acp, acp, s));              // (waits for s: the set is complete before any lane reads it)
    c->car_acp_comb = c->cur.tii_comb;
    c->car_acp_pattern = c->cur.tii_pattern;
    return DABGPU_OK;
}

// coded bits -> carriers (carriers_from_bits_kernel) for n_frames frames of the stream, from the TII parity as it stands
int run_carriers(dabgpu_ctx *c, const void *d_bits, size_t n_frames, float2 *d_car, bool cic, hipStream_t s)
{
    CarrierArgs a{};
    a.g = c->g;
    a.t = tables_of(c);
    a.bits = (const uint8_t *)d_bits;
    a.out = d_car;
    a.n_frames = (int)n_frames;
    a.cic = cic ? (const float *)c->d_cic_chain.p : nullptr;
    if (c->cur.tii_enable && (c->g.mode == 1 || c->g.mode == 2)) {
        const int rc = ensure_carrier_acp(c, s);
        if (rc) return rc;
        a.acp = (const uint8_t *)c->d_car_acp.p;
        a.tii_old_variant = c->cur.tii_old_variant ? 1 : 0;
        a.tii_insert0 = c->tii_insert ? 1 : 0;
    }
    HIPCHK(c, launch_carriers_from_bits(a, s));
    return DABGPU_OK;
}

// The front kernel of a carriers-first plan: *d_in (coded bits, or the caller's carriers) -> d_car, which *d_in then names.
// CicEqualizer sits behind cifSig (src/DabModulator.cpp:399), so carriers handed in are equalised as they are.
int run_front(dabgpu_ctx *c, const ChainPlan &p, const void **d_in, hipStream_t s)
{
    if (p.front == ChainPlan::FRONT_NONE) return DABGPU_OK;
    HIPCHK(c, c->d_car.reserve(p.scratch.d_car));
    float2 *car = (float2 *)c->d_car.p;
    if (p.front == ChainPlan::FRONT_BITS) {
        const int rc = run_carriers(c, *d_in, p.n_frames, car, true, s);
        if (rc) return rc;
    } else {
        HIPCHK(c, launch_cic((const float2 *)*d_in, p.n_frames * (size_t)(c->g.nb_symbols + 1) * (size_t)c->g.K, c->g.K,
                             (const float *)c->d_cic_chain.p, car, s));
    }
    *d_in = car;
    return DABGPU_OK;
}

// The tail of the chain, cifRes -> cifPoly (src/DabModulator.cpp:403-419), on n samples at d_in into d_out (n_out samples):
// the polynomial predistorter is an epilogue of the x2 / x4 resampler's store (fuse_poly; LUT mode is not), otherwise a kernel
// of its own behind it, reading the resampled stream from d_b (d_b_bytes: what the caller's plan sized it to).
int run_tail(dabgpu_ctx *c, unsigned mask, bool fuse_poly, const float2 *d_in, size_t n, float2 *d_out, size_t n_out,
             size_t d_b_bytes, hipStream_t s, unsigned long long *s16_clipped)
{
    int rc;
    if (mask & DABGPU_STAGE_RESAMPLE) {
        float2 *dst = d_out;
        if ((mask & DABGPU_STAGE_POLY) && !fuse_poly) {
            HIPCHK(c, c->d_b.reserve(d_b_bytes));
            dst = (float2 *)c->d_b.p;
        }
        if ((rc = run_resampler(c, d_in, n, dst, s, fuse_poly, s16_clipped))) return rc;
        if (dst == d_out) return DABGPU_OK;
        d_in = dst;
    }
    return (mask & DABGPU_STAGE_POLY) ? run_poly(c, d_in, n_out, d_out, s) : DABGPU_OK;
}

// One chain call as planned: d_in (coded bits or carriers) -> d_out_v, on stream s with lane's scratch.
int run_chain(dabgpu_ctx *c, const ChainPlan &p, const void *d_in, void *d_out_v, size_t out_cap, size_t *out_bytes,
              hipStream_t s, bool apply_format, int lane)
{
    int rc;
    LaneScope scratch(c, lane);
    if (c->cur.cfr_enable) c->cfr_last_lane = lane;   // (also the OfdmGenerator stage wrapper: ITS statistics are the most recent)
    if (p.error) return fail(c, DABGPU_E_INVALID, p.error);
    if ((rc = check_out(c, p.out_bytes, out_cap, out_bytes))) return rc;
    const size_t n_frames = p.n_frames, native = p.native, per = p.per;
    if (n_frames == 0) return DABGPU_OK;

    unsigned long long *clip = nullptr;
    if (apply_format) c->clip_valid = p.fmt != 0;       // (a complexf call leaves no count behind: never the previous call's)
    if (p.fmt) {
        HIPCHK(c, c->d_clip.reserve(16));
        HIPCHK(c, hipMemsetAsync(c->d_clip.p, 0, 16, s));
        clip = (unsigned long long *)c->d_clip.p;
        c->clip_stream = s;
        c->clip_lane = lane;
    }
    // where the chain's last kernel writes: the caller's buffer, or d_fmt in front of the separate convert kernel
    float2 *d_out = (float2 *)d_out_v;
    if (p.scratch.d_fmt) {
        HIPCHK(c, c->d_fmt.reserve(p.scratch.d_fmt));
        d_out = (float2 *)c->d_fmt.p;
    }
    const bool post = p.mask & (DABGPU_STAGE_RESAMPLE | DABGPU_STAGE_POLY);
    if (post) HIPCHK(c, c->d_a.reserve(p.scratch.d_a));
    // carriers first (the CIC equaliser): from here on d_in names the equalised carriers and p the from-carriers chain
    if ((rc = run_front(c, p, &d_in, s))) return rc;

    if (p.piece) {
        // the hand-over in pieces: a two-piece ring in d_a, the producer (every piece with a plan of its own) on lane 1's stream
        const size_t piece = p.piece;
        hipStream_t prod;
        if ((rc = lane_stream(c, 1, &prod))) return rc;
        if (!c->ho_start) {
            HIPCHK(c, hipEventCreateWithFlags(&c->ho_start, hipEventDisableTiming));
            for (int i = 0; i < 2; ++i) {
                HIPCHK(c, hipEventCreateWithFlags(&c->ho_prod[i], hipEventDisableTiming));
                HIPCHK(c, hipEventCreateWithFlags(&c->ho_cons[i], hipEventDisableTiming));
            }
        }
        // the producer starts after whatever the caller queued on s (the input; the previous call's use of the ring)
        HIPCHK(c, hipEventRecord(c->ho_start, s));
        HIPCHK(c, hipStreamWaitEvent(prod, c->ho_start, 0));
        const size_t in_per = p.from_bits ? tf_in_bytes(c->g) : (size_t)(c->g.nb_symbols + 1) * (size_t)c->g.K * sizeof(float2);
        const size_t bps = bytes_per_sample(p.fuse_post ? p.fmt : 0);
        const unsigned native_mask = p.mask & ~(unsigned)(DABGPU_STAGE_RESAMPLE | DABGPU_STAGE_POLY);
        ChainPlan pp = plan_chain(c, p.from_bits, piece, native_mask, false, false);
        size_t f0 = 0;
        for (int i = 0; f0 < n_frames; ++i, f0 += piece) {
            const size_t nf = std::min(piece, n_frames - f0);
            if (nf != piece) pp = plan_chain(c, p.from_bits, nf, native_mask, false, false);   // (the batch's last, shorter piece)
            const int slot = i & 1;
            float2 *ring = (float2 *)c->d_a.p + (size_t)slot * piece * native;
            if (i >= 2) HIPCHK(c, hipStreamWaitEvent(prod, c->ho_cons[slot], 0));   // the consumer is done with piece i - 2
            if ((rc = run_native(c, pp, (const char *)d_in + f0 * in_per, ring, prod))) return rc;
            HIPCHK(c, hipEventRecord(c->ho_prod[slot], prod));
            HIPCHK(c, hipStreamWaitEvent(s, c->ho_prod[slot], 0));
            if ((rc = run_resampler(c, ring, nf * native, (float2 *)((char *)d_out + f0 * per * bps), s, p.fuse_poly,
                                    p.fuse_post ? clip : nullptr)))
                return rc;
            HIPCHK(c, hipEventRecord(c->ho_cons[slot], s));
        }
    } else {
        float2 *native_out = post ? (float2 *)c->d_a.p : d_out;       // where the native-rate stream goes
        if ((rc = run_native_tii(c, p, d_in, native_out, s))) return rc;
        if (post && (rc = run_tail(c, p.mask, p.fuse_poly, native_out, n_frames * native, d_out, n_frames * per, p.scratch.d_b, s,
                                   p.fuse_post ? clip : nullptr)))
            return rc;
    }
    // the insert flag toggles once per frame of the stream whether or not TII is enabled (src/TII.cpp:241-242)
    if ((p.from_bits || p.front == ChainPlan::FRONT_BITS) && (n_frames & 1)) c->tii_insert = !c->tii_insert;
    if (p.scratch.d_fmt) HIPCHK(c, launch_format((const float *)d_out, 2 * n_frames * per, p.fmt, d_out_v, clip, s));
    return DABGPU_OK;
}

}  // namespace dabgpu_api

extern "C" {
// ---- chain -------------------------------------------------------------------

size_t dabgpu_chain_out_bytes_per_frame(const dabgpu_ctx *c, unsigned mask)
{
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(const_cast<dabgpu_ctx *>(c)->mu);
    return out_samples_per_frame(c->g, c->set, mask) * bytes_per_sample(c->set.out_format);
}

int dabgpu_chain_process_dev(dabgpu_ctx *c, const void *d_bits, size_t n_frames, unsigned mask,
                             void *d_iq, size_t out_cap, size_t *out_bytes, void *stream)
{
    CTXCHK(c);
    return chain_dev(c, d_bits, true, n_frames, mask, d_iq, out_cap, out_bytes, stream);
}

int dabgpu_symbols_process_dev(dabgpu_ctx *c, const void *d_car, size_t n_frames, unsigned mask,
                               void *d_iq, size_t out_cap, size_t *out_bytes, void *stream)
{
    CTXCHK(c);
    return chain_dev(c, d_car, false, n_frames, mask, d_iq, out_cap, out_bytes, stream);
}

// coded bits -> carriers: cifMap ... cifSig [-> cifCicEq] by itself (src/DabModulator.cpp:385-399)
int dabgpu_carriers_process_dev(dabgpu_ctx *c, const void *d_bits, size_t n_frames, void *d_carriers, size_t out_cap,
                                size_t *out_bytes, void *stream)
{
    CTXCHK(c);
    int rc = apply_settings(c);
    if (rc) return rc;
    const size_t need = n_frames * (size_t)(c->g.nb_symbols + 1) * (size_t)c->g.K * sizeof(float2);
    if ((rc = check_out(c, need, out_cap, out_bytes))) return rc;
    if (n_frames == 0) return DABGPU_OK;
    if (!d_bits || !d_carriers) return fail(c, DABGPU_E_INVALID, "null argument");
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    if ((rc = run_carriers(c, d_bits, n_frames, (float2 *)d_carriers, chain_cic(c), call.s))) return rc;
    if (n_frames & 1) c->tii_insert = !c->tii_insert;          // like a chain call (src/TII.cpp:241-242)
    return DABGPU_OK;
}

int dabgpu_carriers_process(dabgpu_ctx *c, const uint8_t *bits, size_t in_bytes, void *out, size_t out_cap, size_t *out_bytes)
{
    CTXCHK(c);
    const size_t per = tf_in_bytes(c->g);
    if (!bits || in_bytes == 0 || in_bytes % per)
        return fail(c, DABGPU_E_INVALID, "carriers: input size not valid (whole transmission frames of coded bits)");
    const size_t n_frames = in_bytes / per;
    if (n_frames > (size_t)c->max_frames) return fail(c, DABGPU_E_CAPACITY, "n_frames exceeds max_frames of the context");
    const size_t need = n_frames * (size_t)(c->g.nb_symbols + 1) * (size_t)c->g.K * sizeof(float2);
    int rc = check_out(c, need, out_cap, out_bytes);
    if (rc) return rc;
    if ((rc = dabgpu_synchronize(c))) return rc;               // (d_in / d_out are the synchronous host path's)
    HostIO io(c);
    if ((rc = io.in(c->d_in, bits, in_bytes))) return rc;
    HIPCHK(c, c->d_out.reserve(need));
    size_t ob = 0;
    if ((rc = dabgpu_carriers_process_dev(c, c->d_in.p, n_frames, c->d_out.p, need, &ob, c->stream))) return rc;
    return io.out(out, c->d_out.p, need);
}

// cifRes -> cifPoly on a native-rate stream that is already in device memory: the tail of the chain by itself
int dabgpu_post_process_dev(dabgpu_ctx *c, const void *d_native, size_t n_samples, unsigned mask, void *d_iq, size_t out_cap,
                            size_t *out_bytes, void *stream)
{
    CTXCHK(c);
    int rc = apply_settings(c);
    if (rc) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (!stream && (rc = own_stream_joins_lanes(c))) return rc;     // (d_native: a chain call's output on any lane)
    if (mask & ~(unsigned)(DABGPU_STAGE_RESAMPLE | DABGPU_STAGE_POLY))
        return fail(c, DABGPU_E_INVALID, "post-processing: DABGPU_STAGE_RESAMPLE and / or DABGPU_STAGE_POLY");
    mask = normalised_mask(c->cur, mask);
    size_t n_out = n_samples;
    if (mask & DABGPU_STAGE_RESAMPLE) {
        if ((rc = check_resampler(c))) return rc;
        if (n_samples % ((size_t)c->rs_nin / 2)) return fail(c, DABGPU_E_INVALID, "Resampler::process input size not valid!");
        n_out = n_samples * c->rs_L / c->rs_M;
    }
    if ((rc = check_out(c, n_out * sizeof(float2), out_cap, out_bytes))) return rc;
    if (n_samples == 0) return DABGPU_OK;
    TraceScope trace(c->trace_enabled ? &c->last_variant : nullptr);
    if (!mask) {                                          // (neither stage: the stream passes through)
        HIPCHK(c, hipMemcpyAsync(d_iq, d_native, n_samples * sizeof(float2), hipMemcpyDeviceToDevice, s));
        return DABGPU_OK;
    }
    return run_tail(c, mask, poly_in_resampler(c, mask), (const float2 *)d_native, n_samples, (float2 *)d_iq, n_out,
                    n_out * sizeof(float2), s, nullptr);
}

int dabgpu_chain_process(dabgpu_ctx *c, const uint8_t *bits, size_t n_frames, unsigned mask,
                         void *iq_out, size_t out_cap, size_t *out_bytes)
{
    CTXCHK(c);
    if (n_frames > (size_t)c->max_frames)
        return fail(c, DABGPU_E_CAPACITY, "n_frames exceeds max_frames of the context");
    c->clip_from_collect = false;
    int rc = apply_settings(c);
    if (rc) return rc;
    const ChainPlan p = plan_chain(c, true, n_frames, mask, true, true, chain_cic(c));
    const size_t need = p.out_bytes;
    if (!p.error)
        if (const char *why = monitor_refusal(c, p)) return fail(c, DABGPU_E_INVALID, why);
    if ((rc = check_out(c, need, out_cap, out_bytes))) return rc;
    HostIO io(c);
    if ((rc = io.in(c->d_in, bits, n_frames * tf_in_bytes(c->g)))) return rc;
    // final output lives in its own buffer: d_a / d_b / d_c are the chain's scratch
    HIPCHK(c, c->d_out.reserve(std::max<size_t>(need, 16)));
    size_t ob = 0;
    {
        TraceScope trace(c->trace_enabled ? &c->last_variant : nullptr);
        rc = run_chain(c, p, c->d_in.p, c->d_out.p, need, &ob, c->stream);
        if (!rc) rc = run_monitor(c, p, c->d_in.p, c->d_out.p, c->stream);
        if (!rc) rc = run_spectrum_monitor(c, p, c->d_out.p, c->stream);
    }
    if (rc) return rc;
    return io.out(iq_out, c->d_out.p, need);
}

#ifdef DABGPU_PHASE_TIMING
// tool builds only (tools/phase_timing.py): the frame kernel's per-phase shader-cycle sums since the last call, 16 words
// (Phase order of device_common.h; word 15 = wave-iterations behind the sums); zeroes them
DABGPU_API int dabgpu_debug_phase_cycles(dabgpu_ctx *c, unsigned long long *out16)
{
    CTXCHK(c);
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(out16, c->d_phase.p, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemset(c->d_phase.p, 0, 16 * sizeof(unsigned long long)));
    return DABGPU_OK;
}
#endif

}  // extern "C"
