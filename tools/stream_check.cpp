// stream_check.cpp -- what the streamed stages' entry points are built from (odr-dabmod_amd/csrc/dabgpu_ctx.h: check_stream_call,
// StreamHistory, stream_from_host, stream_reset / _position / _run_samples) on the host alone.  The HIP calls they make, the
// history launch and fail() are fakes defined here: device memory is malloc's, the history kernel is a loop.  No HIP library
// is linked.  Held here, at the bounds: which refusal wins when several apply, n = 2^40, the position at its bound, adjacent
// and overlapping buffers, *n_out on a capacity refusal, and the history a chunked stream leaves behind.  The stages' count_of
// functions live in their own translation units and are not reached from here.
//   c++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include -Iinclude -Iodr-dabmod_amd/csrc tools/stream_check.cpp  (tests/test_stream_host.py)
#include "dabgpu_ctx.h"

namespace {
int g_failed = 0, g_memsets = 0, g_launches = 0, g_code = 0;
std::string g_msg;

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "%s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, g_msg.c_str()); \
            ++g_failed;                                                            \
        }                                                                          \
    } while (0)
}  // namespace

extern "C" {
hipError_t hipMalloc(void **ptr, size_t size) { return (*ptr = std::malloc(size)) ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void *ptr) { std::free(ptr); return hipSuccess; }
hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) { ++g_memsets; std::memset(p, v, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) { std::memcpy(d, s, n); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
int dabgpu_synchronize(dabgpu_ctx *) { return DABGPU_OK; }
}
namespace dabgpu_api {
int fail(dabgpu_ctx *, int code, const std::string &msg) { g_code = code; g_msg = msg; return code; }
int hip_fail(dabgpu_ctx *c, hipError_t, const char *what) { return fail(c, DABGPU_E_DEVICE, what); }
}  // namespace dabgpu_api
namespace dabgpu {
// stream_history_kernel<0> as a loop
hipError_t launch_stream_history(const void *in, int in_fmt, long long n, int H, const float2 *cur, float2 *next, hipStream_t)
{
    if (!in || !cur || !next || cur == next || n < 1 || in_fmt != 0 || H < 1 || H > kStreamMaxHist) return hipErrorInvalidValue;
    ++g_launches;
    for (int j = 0; j < H; ++j) {
        const long long r = n - H + j;
        next[j] = r >= 0 ? static_cast<const float2 *>(in)[r] : cur[H + r];
    }
    return hipSuccess;
}
}  // namespace dabgpu

using namespace dabgpu_api;

int main()
{
    const StreamRules bounded{"tuner", "n_in", "outputs", "tuner: its own alignment text", 1ULL << 50, "tuner: its position text"};
    const StreamRules open{"channel", "n_samples", "samples", nullptr, 0, nullptr};
    const size_t big = (size_t)1 << 40;
    const char *in = reinterpret_cast<const char *>((uintptr_t)1 << 44);     // (addresses only: nothing is read through them)
    const auto at = [&](long long bytes) { return static_cast<const void *>(in + bytes); };
    StreamStage st;
    size_t made = 777;
    const auto refused = [&](int rc, int code, const char *msg) { return rc == code && g_code == code && g_msg == msg; };

    // ---- the order of the refusals: each line has every later fault as well
    st.position = (1ULL << 50) + 1;
    CHECK(refused(check_stream_call(nullptr, st, bounded, nullptr, 0, 0, at(1), 0, 9, 0, &made), DABGPU_E_INVALID, "null argument"));
    CHECK(refused(check_stream_call(nullptr, st, bounded, in, 0, 0, at(0), 0, 9, 0, nullptr), DABGPU_E_INVALID, "null argument"));
    CHECK(refused(check_stream_call(nullptr, st, bounded, in, 0, 0, at(4), 0, 9, 0, &made), DABGPU_E_INVALID, "tuner: its own alignment text"));
    CHECK(refused(check_stream_call(nullptr, st, open, at(2), DABGPU_FMT_S16, 0, in, 0, 9, 0, &made), DABGPU_E_INVALID,
                  "channel: buffers must be aligned to a sample (eight bytes complexf, four bytes s16)"));
    CHECK(check_stream_call(nullptr, st, bounded, at(2), DABGPU_FMT_U8, 1, at(-8), 0, 1, 1, &made) != DABGPU_OK && g_msg == "tuner: its position text");
    CHECK(refused(check_stream_call(nullptr, st, bounded, in, 0, 0, in, 0, 9, 0, &made), DABGPU_E_INVALID, "tuner: n_in must not be 0"));
    CHECK(refused(check_stream_call(nullptr, st, bounded, in, 0, big + 1, in, 0, 9, 0, &made), DABGPU_E_INVALID, "tuner: n_in must not exceed 2^40"));
    CHECK(refused(check_stream_call(nullptr, st, open, in, 0, big + 1, in, 0, 9, 0, &made), DABGPU_E_INVALID, "channel: n_samples must not exceed 2^40"));
    CHECK(refused(check_stream_call(nullptr, st, bounded, in, 0, 1, in, 0, 9, 0, &made), DABGPU_E_INVALID, "tuner: its position text"));
    CHECK(made == 777);
    st.position = 0;
    CHECK(refused(check_stream_call(nullptr, st, bounded, in, 0, 16, in, 0, 9, 8, &made), DABGPU_E_CAPACITY, "tuner: output buffer too small"));
    CHECK(made == 9);                                                    // (what the caller has to offer, before the refusal)
    made = 777;
    CHECK(refused(check_stream_call(nullptr, st, bounded, in, 0, 16, in, 0, 9, 9, &made), DABGPU_E_INVALID, "tuner: input and output must not overlap"));
    CHECK(made == 777);

    // ---- at the bounds: n = 2^40 ends exactly on the position bound; one more sample of position does not
    st.position = (1ULL << 50) - big;
    CHECK(check_stream_call(nullptr, st, bounded, in, 0, big, at(-8), 0, 1, 1, &made) == DABGPU_OK);
    st.position += 1;
    CHECK(refused(check_stream_call(nullptr, st, bounded, in, 0, big, at(-8), 0, 1, 1, &made), DABGPU_E_INVALID, "tuner: its position text"));
    st.position = ~0ULL - 2;                                             // (the channel's position is any, and wraps)
    CHECK(check_stream_call(nullptr, st, open, in, 0, 7, at(56), 0, 7, 7, &made) == DABGPU_OK);
    // adjacent is fine on either side, one sample into the other is not: 100 complexf in, 50 s16 out
    CHECK(check_stream_call(nullptr, st, open, in, 0, 100, at(800), DABGPU_FMT_S16, 50, 50, &made) == DABGPU_OK);
    CHECK(check_stream_call(nullptr, st, open, in, 0, 100, at(796), DABGPU_FMT_S16, 50, 50, &made) == DABGPU_E_INVALID);
    CHECK(check_stream_call(nullptr, st, open, in, 0, 100, at(-200), DABGPU_FMT_S16, 50, 50, &made) == DABGPU_OK);
    CHECK(check_stream_call(nullptr, st, open, in, 0, 100, at(-196), DABGPU_FMT_S16, 50, 50, &made) == DABGPU_E_INVALID);
    CHECK(check_stream_call(nullptr, st, open, in, 0, big, at((long long)big * 8), 0, big, big, &made) == DABGPU_OK);
    CHECK(check_stream_call(nullptr, st, open, in, 0, big, at((long long)big * 8 - 8), 0, big, big, &made) == DABGPU_E_INVALID);

    // ---- the history: a stream of 200 samples in calls shorter than, equal to and longer than a history of 31 (H = 20 in use)
    {
        dabgpu_ctx c;
        StreamStage s;
        std::vector<float2> x(200);
        for (size_t i = 0; i < x.size(); ++i) x[i] = make_float2((float)i, -(float)i);
        const int capacity = 31, H = 20;
        const size_t lengths[] = {1, 7, 19, 20, 21, 31, 40, 61};
        size_t done = 0;
        hipStream_t own = reinterpret_cast<hipStream_t>(&c);
        for (size_t n : lengths) {
            StreamHistory h;
            CHECK(h.begin(&c, s, capacity, own) == DABGPU_OK && h.cur != h.next && g_memsets == 1 && !s.zero_pending);
            for (int j = 0; j < H; ++j) {                                // cur: the H samples in front of this call, zero before the stream
                const long long i = (long long)done - H + j;
                CHECK(h.cur[j].x == (i < 0 ? 0.f : (float)i));
            }
            const int cur_was = s.hist_cur;
            CHECK(h.end(&c, s, &x[done], 0, n, capacity + 1, own) == DABGPU_E_DEVICE && s.hist_cur == cur_was && s.position == done);
            CHECK(h.end(&c, s, &x[done], 0, n, H, own) == DABGPU_OK && s.hist_cur == (cur_was ^ 1) && s.stream == own);
            done += n;
            CHECK(s.position == done);
        }
        CHECK(done == x.size() && g_launches == 8);

        // reset, position, run samples
        uint64_t p = 0;
        CHECK(stream_reset(&c, s, bounded, (1ULL << 50) + 1) == DABGPU_E_INVALID && s.position == done && !s.zero_pending);
        CHECK(stream_reset(&c, s, bounded, 1ULL << 50) == DABGPU_OK && s.zero_pending);
        CHECK(stream_reset(&c, s, open, ~0ULL) == DABGPU_OK && stream_position(&c, s, &p) == DABGPU_OK && p == ~0ULL);
        CHECK(refused(stream_position(&c, s, nullptr), DABGPU_E_INVALID, "null argument"));
        CHECK(refused(stream_run_samples(&c, s, open, -1), DABGPU_E_INVALID, "channel: samples per workgroup must not be negative (0 = chosen)"));
        CHECK(stream_run_samples(&c, s, bounded, 5) == DABGPU_OK && s.run_samples == 5);

        // the host-pointer form: 3 samples in, 2 out, through the stage's staging
        float2 out[2] = {};
        int rc = stream_from_host(&c, s, x.data() + 4, 3 * sizeof(float2), out, sizeof out, [&](const void *d_in, void *d_out) {
            CHECK(d_in == s.in.p && d_out == s.out.p && s.in.cap >= 24 && s.out.cap >= 16);
            std::memcpy(d_out, static_cast<const float2 *>(d_in) + 1, sizeof out);
            return DABGPU_OK;
        });
        CHECK(rc == DABGPU_OK && out[0].x == 5.f && out[1].x == 6.f);
        CHECK(stream_from_host(&c, s, x.data(), 8, out, 8, [&](const void *, void *) { return DABGPU_E_INVALID; }) == DABGPU_E_INVALID);
    }
    if (g_failed) return 1;
    std::printf("stream ok: %d history launches, %d memset\n", g_launches, g_memsets);
    return 0;
}
