// api_channel.hip -- the channel emulator of channel.hip behind the C-ABI: a sparse, time-varying multipath channel with seeded
// Gaussian noise on a sample stream (dabgpu_set_channel, dabgpu_channel / _dev), the stream's history and position
// (dabgpu_channel_reset, dabgpu_get_channel_position) and the settings check (dabgpu_channel_check, host only).  The reference
// has no such stage: nothing here replaces a plugin of its flowgraph, which is why no entry is named *_process.
#include "dabgpu_ctx.h"

using namespace dabgpu;
using namespace dabgpu_api;

static_assert(DABGPU_CH_MAX_PATHS == kChMaxPaths && DABGPU_CH_MAX_DELAY == kChMaxDelay, "the header's limits are the kernel's");

namespace {
constexpr StreamRules kRules{"channel", "n_samples", "samples", nullptr, 0, nullptr};       // (any reset position)

// the refusals that depend on the settings alone (dabgpu_channel_check: no context, no device); nullptr = fine
const char *settings_refusal(const dabgpu_channel_config *cfg)
{
    if (!cfg) return "null argument";
    if (cfg->n_paths > (uint32_t)kChMaxPaths) return "channel: at most 64 paths (DABGPU_CH_MAX_PATHS)";
    if (!std::isfinite(cfg->sigma)) return "channel: gains and sigma must be finite";
    if (cfg->sigma < 0.f) return "channel: sigma must not be negative";
    if (!(cfg->rate_hz > 0.0) || !std::isfinite(cfg->rate_hz)) return "channel: rate_hz must be positive";
    for (uint32_t p = 0; p < cfg->n_paths; ++p) {
        const dabgpu_channel_path &q = cfg->paths[p];
        if (q.delay > (uint32_t)kChMaxDelay) return "channel: a path's delay is 0 ... 2047 samples (DABGPU_CH_MAX_DELAY)";
        if (!std::isfinite(q.gain_re) || !std::isfinite(q.gain_im)) return "channel: gains and sigma must be finite";
        if (!(std::fabs(q.doppler_hz) < cfg->rate_hz / 2)) return "channel: |doppler_hz| must be below rate_hz / 2";
    }
    return nullptr;
}

// rint(doppler_hz / rate_hz 2^64) as a two's-complement 64-bit integer (|.| < 2^63: the signed conversion is defined)
unsigned long long doppler_step(double doppler_hz, double rate_hz)
{
    return (unsigned long long)(long long)std::rint(doppler_hz / rate_hz * 18446744073709551616.0);
}

int check_call(dabgpu_ctx *c, const void *in, int in_format, size_t n_samples, const void *out, int out_format)
{
    if (!c->channel.configured) return fail(c, DABGPU_E_INVALID, "channel: no configuration (no dabgpu_set_channel call yet)");
    if ((in_format != 0 && in_format != DABGPU_FMT_S16) || (out_format != 0 && out_format != DABGPU_FMT_S16))
        return fail(c, DABGPU_E_INVALID, "channel: formats are complexf (0) or DABGPU_FMT_S16");
    size_t made;                          // (as many outputs as inputs: the capacity is never short)
    return check_stream_call(c, c->channel, kRules, in, in_format, n_samples, out, out_format, n_samples, n_samples, &made);
}
}  // namespace

extern "C" {
int dabgpu_channel_check(const dabgpu_channel_config *cfg)
{
    if (const char *why = settings_refusal(cfg)) return fail(nullptr, DABGPU_E_INVALID, why);
    return DABGPU_OK;
}

int dabgpu_set_channel(dabgpu_ctx *c, const dabgpu_channel_config *cfg)
{
    CTXCHK(c);
    if (const char *why = settings_refusal(cfg)) return fail(c, DABGPU_E_INVALID, why);
    ChannelArgs a{};
    a.sigma = cfg->sigma;
    a.seed_lo = (uint32_t)cfg->seed;
    a.seed_hi = (uint32_t)(cfg->seed >> 32);
    // the paths that do not rotate first, either group in the given order (the two sums of the definition)
    for (int rotating = 0; rotating < 2; ++rotating) {
        for (uint32_t p = 0; p < cfg->n_paths; ++p) {
            const dabgpu_channel_path &q = cfg->paths[p];
            const unsigned long long step = doppler_step(q.doppler_hz, cfg->rate_hz);
            if ((step != 0) != (rotating != 0)) continue;
            ChannelPath &d = a.path[a.n_paths++];
            d.delay = q.delay;
            d.gr = q.gain_re;
            d.gi = q.gain_im;
            d.step = step;
        }
        if (!rotating) a.n_static = a.n_paths;
    }
    c->channel.args = a;
    c->channel.configured = true;
    return DABGPU_OK;
}

int dabgpu_channel_reset(dabgpu_ctx *c, uint64_t position)
{
    CTXCHK(c);
    return stream_reset(c, c->channel, kRules, position);
}

int dabgpu_get_channel_position(dabgpu_ctx *c, uint64_t *position)
{
    CTXCHK(c);
    return stream_position(c, c->channel, position);
}

int dabgpu_debug_channel_run_samples(dabgpu_ctx *c, int samples)
{
    CTXCHK(c);
    return stream_run_samples(c, c->channel, kRules, samples);
}

int dabgpu_channel_dev(dabgpu_ctx *c, const void *d_in, int in_format, size_t n_samples, void *d_out, int out_format, void *stream)
{
    CTXCHK(c);
    int rc = check_call(c, d_in, in_format, n_samples, d_out, out_format);
    if (rc) return rc;
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    StreamHistory h;
    if ((rc = h.begin(c, c->channel, kChMaxDelay, call.s))) return rc;
    ChannelArgs a = c->channel.args;
    a.in = d_in;
    a.out = d_out;
    a.hist = h.cur;
    a.n = (long long)n_samples;
    a.position = c->channel.position;
    a.in_fmt = in_format ? 1 : 0;
    a.out_fmt = out_format ? 1 : 0;
    a.run = channel_run(n_samples, c->channel.run_samples);
    HIPCHK(c, launch_channel(a, call.s));
    return h.end(c, c->channel, d_in, in_format, n_samples, kChMaxDelay, call.s);
}

int dabgpu_channel(dabgpu_ctx *c, const void *in, int in_format, size_t n_samples, void *out, int out_format)
{
    CTXCHK(c);
    int rc = check_call(c, in, in_format, n_samples, out, out_format);
    if (rc) return rc;
    return stream_from_host(c, c->channel, in, n_samples * sample_bytes(in_format), out, n_samples * sample_bytes(out_format),
                            [&](const void *d_in, void *d_out) {
                                return dabgpu_channel_dev(c, d_in, in_format, n_samples, d_out, out_format, c->stream);
                            });
}

}  // extern "C"
