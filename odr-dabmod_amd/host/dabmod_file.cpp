// dabmod_file -- ETI file in, IQ file out: BASELINE config 1 ("Mode I, native 2.048 Msps, ETI file ->
// IQ file") as one command, the file-to-file shape of the reference's odr-dabmod
// (src/DabMod.cpp:365-520 for the wiring, doc/example.ini for the options).
//
//   InputFileReader -> EtiFrontend (CPU: ETI -> coded bits)        odr-dabmod_amd/host/Frontend.h
//                   -> DabGpuChain (MI355X: coded bits -> IQ)       odr-dabmod_amd/host/GpuStages.h
//                   -> [FormatConverter] -> file
// or, with --gpu-frontend, the front-end on the device as well (DabGpuChain::submit_eti):
//   InputFileReader -> DabGpuChain (MI355X: ETI frames -> coded bits -> IQ) -> file
//
// usage: dabmod_file <in.eti> <out> [options]
//   --mode N             transmission mode 1..4 (default: from the ETI header, 0 -> 4)
//   --format F           complexf (default) | s16 | u8 | s8
//   --gainmode M         var (default) | fix | max        --digital G   --normalise X   --var V
//   --fir none|default|<tapsfile>      (default: none, as config 1)
//   --rate R             output sample rate (default 2048000)
//   --poly <coeffile>    MemlessPoly coefficient file
//   --ofdmwindowing W    raised-cosine overlap in samples
//   --tii comb,pattern   --cfr clip,errorclip
//   --cic SPACING,R      CicEqualizer(carriers, SPACING, R) between the signal multiplexer and OfdmGenerator, what the reference
//                        wires in for a configured dac_clk_rate (src/DabModulator.cpp:155-176): the chain runs carriers first
//   --loop N             read the file N times
//   --bits-only          stop after the front-end: write the hot path's input blocks (no GPU needed)
//   --reference-latency  emit exactly the frames the reference emits: one transmission frame fewer per pipelined stage
//                        of the equivalent reference graph (GainControl, FIRFilter, MemlessPoly: src/ModPlugin.cpp:90-115)
//   --reference-gain     gain mode var: the reference's running fp32 recurrence (src/GainControl.cpp:251-340) instead of the
//                        exact variance (DabGpuChain::Settings::referenceGainRounding)
//   --contexts N         with --batch B > 1: the batches of the stream go to N chains (1 ... 4, default 1) on the same device in
//                        turn, batch j to chain j mod N, which is first seeded from the last frame of batch j - 1
//                        (DabGpuChain::seed): the same bytes as one chain, the chains' kernels side by side
//                        (N > 1 needs the streaming path: not with --bits-only or --separate-converter)
//   --gpu-frontend       ETI frames go to the device as they are (DabGpuChain::configure_frontend / submit_eti): the program
//                        skips frames until FP = 0, reads the multiplex layout from that frame and hands whole batches of ETI
//                        frames over (--batch transmission frames each, default 1).  The same file as without the option.
//                        The library wants the frame phase of every call's first frame aligned to the transmission frame:
//                        on a stream whose FP jumps (the CPU front-end never looks at FP after the start) the program
//                        stops with that message.  Not with --contexts above 1 (the time interleaver's history is not part of the stream state a
//                        chain is seeded with), --bits-only or --separate-converter.
//   --monitor            the receiver behind every GPU call (DabGpuChain::Settings::monitor): every frame written is decoded on the
//                        device against the coded bits it was made from.  After the run: frames, bit errors, worst and mean MER
//                        on stderr; exit status 2 when a bit error was counted.  The output file is the one without the option.
//                        Native-rate complexf / s16 output; with --batch the batches run one at a time.
//   --loopback           with --gpu-frontend: the whole loop closed on the device.  After each batch its IQ is demodulated
//                        (dabgpu_demod, the window where --monitor puts it) and the coded bits are decoded (dabgpu_decode: time
//                        de-interleaver, Viterbi, energy dispersal) against the ETI frames the program read, which it keeps in
//                        a ring of fifteen: the decoder returns a frame fifteen frames after its first bits went out, and
//                        never returns the last fifteen of the file.  After the run: frames compared, FIC and MSC payload
//                        bit errors, corrected channel bits and coded bits on stderr; exit status 2 on any payload bit error.
//                        Native-rate complexf / s16 output; not with --state-in (the decoder's history is not in the file).
//   --blind              with --loopback: the receiving side knows nothing of the file's layout.  It decodes on a context of its
//                        own, configured with dabgpu_fic_bootstrap_frame (NST = 0: the FIC alone).  It reads the FIC of the
//                        first batch (dabgpu_fic_scan on the decoder's output), configures itself from it
//                        (dabgpu_decode_configure_from_fic) and decodes that batch again from its start; every later batch is
//                        decoded as --loopback does.  Prints the FIBs good / bad / zero, the EId and the sub-channel table it
//                        found.  The first batch must hold more than fifteen ETI frames (--batch), and the file's FIC must be
//                        a real one that numbers the sub-channels as the STC words do.  Exit status 4 when no configuration
//                        could be read, or when it is not the file's; 2 on a payload bit error, as --loopback.  Hard decisions
//                        only (not with --soft).
//   --soft               with --loopback: soft decisions -- dabgpu_demod_soft (one int8 metric per coded bit) and
//                        dabgpu_decode_soft in place of the hard pair, the same bookkeeping and exit status.  The summary line
//                        adds the path metric over the sum of the metrics' magnitudes, and the erasures.  On the modulator's
//                        own clean output the metric is 0: the option makes the path reachable from the program.
//   --channel-cn DB      with --loopback: the channel emulator (dabgpu_channel) between the batch's IQ and the demodulator: Gaussian
//                        noise DB below the mean power of the first batch's samples behind the null symbol (computed once),
//                        from --channel-seed N (default 0); one stream position runs across the batches.  --channel-echo
//                        DELAY,DB,PHASE (repeatable) adds a path behind the direct one: DELAY samples late, DB relative to it,
//                        PHASE radians.  Echoes inside the guard interval need no synchroniser -- the window is where --monitor
//                        puts it -- so a DELAY above the cyclic prefix less that window's lead is refused (at the first batch,
//                        when the filter's length is known: exit status 1, as every failure of the run).  No carrier offset
//                        here (that takes the synchroniser across batch boundaries).  The summary adds C/N, seed and paths; the
//                        output file is the one without the options; exit statuses as --loopback's.
//   --spectrum FILE      the spectrum monitor behind every GPU call (DabGpuChain::Settings::spectrum): a Welch power spectrum of
//                        everything written -- any rate, any format -- 2048 bins, Blackman-Harris window.  After the run FILE
//                        holds one "offset_hz level_db" line per bin in ascending frequency, level relative to the mean over
//                        the occupied band (+-768 kHz); stderr gets the segments and the out-of-band maximum (from --oob-from
//                        HZ, default 970000) with its frequency.  The output file is the one without the option.  With
//                        --contexts N the contexts' sums are added.  Not with --bits-only or --separate-converter.
//   --dpd-feedback RXFILE --dpd-out COEFFILE [--dpd-bins N] [--dpd-min-count N]
//                        the DPD measurement (include/dabgpu.h, "DPD measurement"): RXFILE holds complexf samples of the
//                        amplifier's feedback path, sample i belonging to sample i of this run's output stream up to an unknown
//                        delay (|delay| <= 1000 samples).  The first batch written gives the alignment (stderr: lag, tau, gain,
//                        coherence) and the peak (its largest |t|); every batch is measured into one set of sums; after the
//                        run the polynomial is fitted (DABGPU_DPD_BASIS_MAGSQ, weighted) and written to COEFFILE in
//                        MemlessPoly's coefficient file format 1, which --poly reads back.  Output complexf or s16 at any
//                        rate; not with --contexts above 1, --bits-only or --separate-converter.  Exit status 4 when the fit
//                        is refused.  N bins (default 64), bins with fewer than --dpd-min-count samples (default 10) unused.
//   --mask MASKFILE      with --spectrum: "offset_hz limit_db" per line (# starts a comment), offsets increasing; the limit is
//                        piecewise linear in dB between the points (dabgpu_spectrum_check_mask).  stderr gets the worst margin
//                        and where it lies; exit status 3 when a bin lies above the mask (2 stays the monitor's).
//   --tii-scan           the TII analyser (dabgpu_tii_scan; include/dabgpu.h, "the TII analyser") on the last batch of two frames
//                        or more that was written, the window where --monitor puts it, min_ratio 12, min_rel 1e-3.  stderr gets
//                        the head and one line per entry (comb, pattern, mask, level, delay); exit status 2 when --tii is given
//                        and the entries are not exactly the one configured -- the comb, and the pattern as the standard reads
//                        it: in Mode II the configured pattern with bits b and b + 4 exchanged.  Native-rate
//                        complexf / s16 output with --batch 2 or more; not with --bits-only or --separate-converter.
//   --cir FILE           the channel estimator (dabgpu_cir; include/dabgpu.h, "the channel estimator") on the last batch that was
//                        written, the window where --monitor puts it, Hann weights, min_ratio 20, min_rel 1e-3.  With
//                        --loopback --channel-cn it is that batch behind the channel emulator instead, so --channel-echo
//                        37,-6,1.0 --cir out.txt shows the echo it was given.  stderr gets the head and one line per path (delay,
//                        level in dB below the strongest, fine); FILE one line per tap: "delay_samples level_db", the level
//                        relative to the peak, in ascending delay.  A measurement, not a verdict: the exit status stays what
//                        it is without the option.  Native-rate complexf / s16 output; not with --bits-only or
//                        --separate-converter.
//   --csi                with --loopback --soft: the soft metrics weighted by the state of their carrier (dabgpu_demod_csi;
//                        include/dabgpu.h, "the carrier state") in place of dabgpu_demod_soft; everything else as --soft.
//   --superframe N       with --loopback: the superframe reader (dabgpu_superframe; include/dabgpu.h, "the superframe reader") on
//                        sub-channel N (in STC order) of every batch's decoded images behind the fifteen of the lead-in, the
//                        last four images carried into the next batch so that every alignment of five is looked at once.  After
//                        the run: candidates, superframes found by the greedy walk over all of them, AUs ok / bad, RS bytes
//                        corrected and words failed on stderr.  WITH THE OPTION THE RUN'S VERDICT IS THE AUs': exit status 2
//                        when an accepted superframe has an AU whose CRC fails, and payload bit errors no longer count -- a
//                        noisy loop passes where the outer code copes.  No superframe at all is no error (exit status 0).
//   --carrier-mer FILE   the per-carrier MER (dabgpu_demod_carrier_state) of the last batch that was written -- with --loopback
//                        --channel-cn of that batch behind the channel emulator, as --cir takes it -- the window where
//                        --monitor puts it.  FILE gets one line per carrier and frame of the batch: "frame position mer_db
//                        weight" (position in frequency order; mer_db 400.000 where no quadrature power was measured); stderr
//                        the median and the lowest MER of the batch.  A measurement, not a verdict.  Native-rate complexf / s16
//                        output; not with --bits-only or --separate-converter.
//   --state-out FILE     with --gpu-frontend: after the last frame, write where the stream stands -- the number of ETI frames
//                        modulated since FP = 0 and both stream-state blobs (DabGpuChain::get_stream_state /
//                        frontend_state) -- so that another run continues it
//   --state-in FILE      with --gpu-frontend: continue the stream a --state-out run left.  The input is the ETI frames that
//                        follow: no skipping to FP = 0, the first frame must open a transmission frame (FP a multiple of
//                        4 / 1 / 1 / 2 in modes I ... IV); the layout is read from it and both blobs are installed.  The
//                        two runs' output files, one behind the other, are the file one run over the whole input writes.
//                        (Both need --gpu-frontend: the CPU front-end's time interleaver is host state the file does not carry.)
#include "Frontend.h"
#include "GpuStages.h"
#include "dabgpu.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace {
// --blind: the receiving side found no configuration in the FIC, or not the file's (exit status 4)
struct BlindFailure : std::runtime_error {
    using std::runtime_error::runtime_error;
};

[[noreturn]] void usage()
{
    std::fprintf(stderr, "usage: dabmod_file <in.eti> <out> [--mode N] [--format complexf|s16|u8|s8] [--gainmode var|fix|max]\n"
                         "       [--digital G] [--normalise X] [--var V] [--fir none|default|file] [--rate R] [--poly file]\n"
                         "       [--ofdmwindowing W] [--tii comb,pattern] [--cfr clip,errorclip] [--cic spacing,R] [--loop N] [--bits-only]\n"
                         "       [--batch N]   N transmission frames per GPU call, two calls in flight (default 1: frame by frame)\n"
                         "       [--reference-latency]   drop the frames the reference's pipelined stages never emit\n"
                         "       [--reference-gain]      gain mode var by the reference's running recurrence (bit-equal scalars, slower)\n"
                         "       [--contexts N]   with --batch B > 1: split the stream's batches over N = 1 ... 4 chains on the device\n"
                         "                        (batch j to chain j mod N, seeded from the frame before it; the same bytes as N = 1;\n"
                         "                        N > 1 not with --bits-only or --separate-converter)\n"
                         "       [--gpu-frontend]   ETI -> coded bits on the device as well (not with --contexts above 1, --bits-only,\n"
                         "                        --separate-converter)\n"
                         "       [--loopback]   with --gpu-frontend: demodulate and channel-decode every batch on the device against the ETI\n"
                         "                        frames read; totals on stderr, exit 2 on a payload bit error\n"
                         "       [--blind]   with --loopback: the decoder configures itself from the FIC of the first batch (exit status 4: it could not)\n"
                         "       [--soft]   with --loopback: soft decisions (int8 metrics, soft Viterbi) in place of hard ones\n"
                         "       [--channel-cn DB [--channel-seed N] [--channel-echo DELAY,DB,PHASE]...]   with --loopback: noise and echoes\n"
                         "           between the IQ and the demodulator (the channel emulator)\n"
                         "       [--monitor]   decode every frame written on the device; totals on stderr, exit 2 on a bit error\n"
                         "       [--dpd-feedback RXFILE --dpd-out COEFFILE [--dpd-bins N] [--dpd-min-count N]]   fit MemlessPoly from a feedback capture\n"
                         "       [--spectrum FILE [--mask MASKFILE] [--oob-from HZ]]   power spectrum of everything written, per bin into FILE;\n"
                         "                        exit 3 when it lies above the mask (lines of: offset_hz limit_db)\n"
                         "       [--tii-scan]   with --batch 2 or more: read the TII of the last batch; exit 2 when it is not the one --tii configures\n"
                         "       [--cir FILE]   impulse response of the channel the last batch went through (with --loopback --channel-cn: the\n"
                         "                        emulator's), per tap into FILE (lines of: delay_samples level_db), paths on stderr\n"
                         "       [--superframe N]   with --loopback: DAB+ superframes of sub-channel N; the exit status is the AU CRCs' (2: a bad AU)\n"
                         "       [--csi]   with --loopback --soft: weight the metrics by the measured state of their carrier\n"
                         "       [--carrier-mer FILE]   MER per carrier of the last batch (lines of: frame position mer_db weight)\n"
                         "       [--state-out FILE] [--state-in FILE]   with --gpu-frontend: leave / take up the stream's state\n");
    std::exit(2);
}

// --state-out / --state-in: "DABMODST", uint64 version 1, uint64 ETI frames modulated since FP = 0, then the front-end blob
// and the chain's stream-state blob, each behind its uint64 length (the blobs describe themselves: include/dabgpu.h)
struct StreamStateFile {
    uint64_t n_eti;
    std::vector<uint8_t> frontend, chain;
};
const char kStateMagic[8] = {'D', 'A', 'B', 'M', 'O', 'D', 'S', 'T'};

void write_state(const std::string &path, const StreamStateFile &st)
{
    std::ofstream f(path, std::ios::binary);
    const uint64_t head[2] = {1, st.n_eti};
    f.write(kStateMagic, sizeof kStateMagic);
    f.write(reinterpret_cast<const char *>(head), sizeof head);
    for (const std::vector<uint8_t> *b : {&st.frontend, &st.chain}) {
        const uint64_t n = b->size();
        f.write(reinterpret_cast<const char *>(&n), sizeof n);
        f.write(reinterpret_cast<const char *>(b->data()), static_cast<std::streamsize>(n));
    }
    if (!f.flush()) throw std::runtime_error("cannot write " + path);
}

StreamStateFile read_state(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    char magic[8];
    uint64_t head[2];
    StreamStateFile st{};
    if (!f.read(magic, sizeof magic) || std::memcmp(magic, kStateMagic, sizeof magic) != 0 ||
        !f.read(reinterpret_cast<char *>(head), sizeof head) || head[0] != 1)
        throw std::runtime_error(path + " is not a stream state written by --state-out");
    st.n_eti = head[1];
    for (std::vector<uint8_t> *b : {&st.frontend, &st.chain}) {
        uint64_t n = 0;
        if (!f.read(reinterpret_cast<char *>(&n), sizeof n) || n > (1u << 24)) throw std::runtime_error(path + " is cut short");
        b->resize(n);
        if (n && !f.read(reinterpret_cast<char *>(b->data()), static_cast<std::streamsize>(n)))
            throw std::runtime_error(path + " is cut short");
    }
    return st;
}
}  // namespace

int main(int argc, char **argv)
{
    if (argc < 3) usage();
    const std::string in_path = argv[1], out_path = argv[2];
    DabGpuChain::Settings gs;
    gs.dabMode = 0;
    std::string format = "complexf";
    bool separate_converter = false;
    int loops = 1;
    bool bits_only = false;
    size_t batch = 1;
    bool reference_latency = false;
    long contexts = 1;
    bool gpu_frontend = false, loopback = false, soft = false, csi = false, blind = false;
    std::string carrier_mer_path;
    long superframe = -1;
    bool channel = false;
    double channel_cn = 0.0;
    unsigned long long channel_seed = 0;
    struct Echo { unsigned delay; double db, phase; };
    std::vector<Echo> channel_echoes;
    std::string state_in, state_out;
    std::string spectrum_path, mask_path;
    double oob_from = 970000.0;
    std::string dpd_rx_path, dpd_out_path;
    int dpd_bins = 64;
    unsigned long dpd_min_count = 10;
    bool tii_scan = false;
    std::string cir_path;
    try {
        for (int i = 3; i < argc; ++i) {
            const std::string a = argv[i];
            auto val = [&]() -> std::string {
                if (i + 1 >= argc) usage();
                return argv[++i];
            };
            if (a == "--mode") gs.dabMode = static_cast<unsigned>(std::stoul(val()));
            else if (a == "--format") format = val();
            else if (a == "--separate-converter") separate_converter = true;
            else if (a == "--gainmode") {
                const std::string m = val();
                gs.gainMode = m == "fix" ? GainMode::GAIN_FIX : m == "max" ? GainMode::GAIN_MAX : GainMode::GAIN_VAR;
            }
            else if (a == "--digital") gs.digitalGain = std::stof(val());
            else if (a == "--normalise") gs.normalise = std::stof(val());
            else if (a == "--var") gs.gainmodeVariance = std::stof(val());
            else if (a == "--fir") { const std::string f = val(); gs.filterTapsFilename = f == "none" ? "" : f; }
            else if (a == "--rate") gs.outputRate = std::stoul(val());
            else if (a == "--poly") gs.polyCoefFilename = val();
            else if (a == "--ofdmwindowing") gs.ofdmWindowOverlap = std::stoul(val());
            else if (a == "--tii") {
                if (std::sscanf(val().c_str(), "%d,%d", &gs.tiiConfig.comb, &gs.tiiConfig.pattern) != 2) usage();
                gs.tiiConfig.enable = true;
            }
            else if (a == "--cfr") {
                if (std::sscanf(val().c_str(), "%f,%f", &gs.cfrClip, &gs.cfrErrorClip) != 2) usage();
                gs.enableCfr = true;
            }
            else if (a == "--cic") {
                unsigned long spacing = 0;
                if (std::sscanf(val().c_str(), "%lu,%d", &spacing, &gs.cicRatio) != 2 || !spacing || gs.cicRatio <= 0) usage();
                gs.cicSpacing = spacing;
            }
            else if (a == "--loop") loops = std::atoi(val().c_str());
            else if (a == "--bits-only") bits_only = true;
            else if (a == "--batch") batch = std::max<size_t>(1, std::stoul(val()));
            else if (a == "--reference-latency") reference_latency = true;
            else if (a == "--reference-gain") gs.referenceGainRounding = true;
            else if (a == "--gpu-frontend") gpu_frontend = true;
            else if (a == "--monitor") gs.monitor = true;
            else if (a == "--loopback") loopback = true;
            else if (a == "--blind") blind = true;
            else if (a == "--soft") soft = true;
            else if (a == "--csi") csi = true;
            else if (a == "--carrier-mer") carrier_mer_path = val();
            else if (a == "--superframe") {
                const std::string v = val();
                size_t used = 0;
                superframe = std::stol(v, &used);
                if (used != v.size() || superframe < 0) usage();
            }
            else if (a == "--channel-cn") { channel_cn = std::stod(val()); channel = true; }
            else if (a == "--channel-seed") channel_seed = std::stoull(val());
            else if (a == "--channel-echo") {
                Echo e{};
                if (std::sscanf(val().c_str(), "%u,%lf,%lf", &e.delay, &e.db, &e.phase) != 3) usage();
                channel_echoes.push_back(e);
            }
            else if (a == "--spectrum") { spectrum_path = val(); gs.spectrum = true; }
            else if (a == "--mask") mask_path = val();
            else if (a == "--oob-from") oob_from = std::stod(val());
            else if (a == "--dpd-feedback") dpd_rx_path = val();
            else if (a == "--dpd-out") dpd_out_path = val();
            else if (a == "--dpd-bins") dpd_bins = std::atoi(val().c_str());
            else if (a == "--dpd-min-count") dpd_min_count = std::stoul(val());
            else if (a == "--tii-scan") tii_scan = true;
            else if (a == "--cir") cir_path = val();
            else if (a == "--state-in") state_in = val();
            else if (a == "--state-out") state_out = val();
            else if (a == "--contexts") {
                const std::string v = val();
                size_t used = 0;
                contexts = std::stol(v, &used);
                if (used != v.size()) usage();
            }
            else usage();
        }
        // (several chains take whole batches of the streaming path in turn: nothing to split frame by frame)
        if (contexts < 1 || contexts > 4 || (contexts > 1 && (batch <= 1 || separate_converter || bits_only))) usage();

        if (gpu_frontend && (contexts > 1 || bits_only || separate_converter)) {
            std::fprintf(stderr, "dabmod_file: --gpu-frontend does not go with %s\n",
                         contexts > 1 ? "--contexts above 1: the front-end's state (the time interleaver's history) is not part of "
                                        "the stream state a chain is seeded with"
                         : bits_only  ? "--bits-only: the coded bits stay on the device"
                                      : "--separate-converter: the streaming path converts inside the chain");
            return 2;
        }

        if (loopback && (!gpu_frontend || gs.outputRate != 2048000 || (format != "complexf" && format != "s16") || !state_in.empty())) {
            std::fprintf(stderr, "dabmod_file: --loopback does not go with %s\n",
                         !gpu_frontend ? "the CPU front-end (it needs --gpu-frontend): the decoder reads the layout the device front-end holds"
                         : gs.outputRate != 2048000 ? "--rate: the receiver takes the native rate"
                         : !state_in.empty() ? "--state-in: the decoder's history is not part of the state file"
                                             : "u8 / s8 output: the receiver takes complexf or s16");
            return 2;
        }

        if (blind && (!loopback || soft)) {
            std::fprintf(stderr, "dabmod_file: --blind does not go %s\n",
                         !loopback ? "without --loopback: it is that loop's receiving side that configures itself"
                                   : "with --soft: the FIC is read from the hard decoder's output");
            return 2;
        }

        if (soft && !loopback) {
            std::fprintf(stderr, "dabmod_file: --soft does not go without --loopback: it chooses the decisions of that loop\n");
            return 2;
        }

        if (superframe >= 0 && !loopback) {
            std::fprintf(stderr, "dabmod_file: --superframe does not go without --loopback: it reads that loop's decoded images\n");
            return 2;
        }

        if (csi && !soft) {
            std::fprintf(stderr, "dabmod_file: --csi does not go without --loopback --soft: it weights the metrics of that loop\n");
            return 2;
        }

        if ((channel || channel_seed || !channel_echoes.empty()) && !(loopback && channel)) {
            std::fprintf(stderr, "dabmod_file: --channel-seed and --channel-echo go with --channel-cn, and that with --loopback: the "
                                 "channel sits between the IQ and that loop's demodulator\n");
            return 2;
        }
        if (channel_echoes.size() + 1 > DABGPU_CH_MAX_PATHS) {
            std::fprintf(stderr, "dabmod_file: --channel-echo: at most %d echoes\n", DABGPU_CH_MAX_PATHS - 1);
            return 2;
        }

        if (gs.monitor && (bits_only || separate_converter)) {
            std::fprintf(stderr, "dabmod_file: --monitor does not go with %s\n",
                         bits_only ? "--bits-only: nothing is modulated" : "--separate-converter: the chain's own output is what is decoded");
            return 2;
        }

        if (tii_scan && (gs.outputRate != 2048000 || (format != "complexf" && format != "s16") || bits_only || separate_converter || batch < 2)) {
            std::fprintf(stderr, "dabmod_file: --tii-scan does not go with %s\n",
                         gs.outputRate != 2048000 ? "--rate: the analyser takes the native rate"
                         : bits_only  ? "--bits-only: nothing is modulated"
                         : separate_converter ? "--separate-converter: the chain's own output is what is scanned"
                         : batch < 2  ? "--batch below 2: the last batch is scanned, and a scan takes two frames or more"
                                      : "u8 / s8 output: the analyser takes complexf or s16");
            return 2;
        }

        const bool cir = !cir_path.empty();
        if (cir && (gs.outputRate != 2048000 || (format != "complexf" && format != "s16") || bits_only || separate_converter)) {
            std::fprintf(stderr, "dabmod_file: --cir does not go with %s\n",
                         gs.outputRate != 2048000 ? "--rate: the estimator takes the native rate"
                         : bits_only  ? "--bits-only: nothing is modulated"
                         : separate_converter ? "--separate-converter: the chain's own output is what is measured"
                                      : "u8 / s8 output: the estimator takes complexf or s16");
            return 2;
        }

        const bool carrier_mer = !carrier_mer_path.empty();
        if (carrier_mer && (gs.outputRate != 2048000 || (format != "complexf" && format != "s16") || bits_only || separate_converter)) {
            std::fprintf(stderr, "dabmod_file: --carrier-mer does not go with %s\n",
                         gs.outputRate != 2048000 ? "--rate: the receiver takes the native rate"
                         : bits_only  ? "--bits-only: nothing is modulated"
                         : separate_converter ? "--separate-converter: the chain's own output is what is measured"
                                      : "u8 / s8 output: the receiver takes complexf or s16");
            return 2;
        }

        if (gs.spectrum && (bits_only || separate_converter)) {
            std::fprintf(stderr, "dabmod_file: --spectrum does not go with %s\n",
                         bits_only ? "--bits-only: nothing is modulated" : "--separate-converter: the chain's own output is what is measured");
            return 2;
        }
        if (!mask_path.empty() && !gs.spectrum) {
            std::fprintf(stderr, "dabmod_file: --mask needs --spectrum\n");
            return 2;
        }
        const bool dpd = !dpd_rx_path.empty();
        if (dpd_rx_path.empty() != dpd_out_path.empty()) {
            std::fprintf(stderr, "dabmod_file: --dpd-feedback and --dpd-out go together\n");
            return 2;
        }
        if (dpd && (contexts > 1 || bits_only || separate_converter || (format != "complexf" && format != "s16"))) {
            std::fprintf(stderr, "dabmod_file: --dpd-feedback does not go with %s\n",
                         contexts > 1 ? "--contexts above 1: one context holds the sums"
                         : bits_only  ? "--bits-only: nothing is modulated"
                         : separate_converter ? "--separate-converter: the chain's own output is what is measured"
                                              : "u8 / s8 output: the transmitted samples are complexf or s16");
            return 2;
        }
        std::ifstream dpd_rx;
        if (dpd) {
            dpd_rx.open(dpd_rx_path, std::ios::binary);
            if (!dpd_rx) {
                std::fprintf(stderr, "dabmod_file: cannot read %s\n", dpd_rx_path.c_str());
                return 1;
            }
        }
        std::vector<double> mask_offs, mask_limit;
        if (!mask_path.empty()) {
            std::ifstream mf(mask_path);
            if (!mf) {
                std::fprintf(stderr, "dabmod_file: cannot read %s\n", mask_path.c_str());
                return 1;
            }
            std::string line;
            while (std::getline(mf, line)) {
                line = line.substr(0, line.find('#'));
                double o, l;
                char rest;
                const int n = std::sscanf(line.c_str(), " %lf %lf %c", &o, &l, &rest);
                if (n == 2) { mask_offs.push_back(o); mask_limit.push_back(l); }
                else if (n != EOF && n != 0) {
                    std::fprintf(stderr, "dabmod_file: %s: a line is \"offset_hz limit_db\"\n", mask_path.c_str());
                    return 1;
                }
            }
            if (mask_offs.empty()) {
                std::fprintf(stderr, "dabmod_file: %s holds no mask point\n", mask_path.c_str());
                return 1;
            }
        }

        if (!gpu_frontend && !(state_in.empty() && state_out.empty())) {
            std::fprintf(stderr, "dabmod_file: %s does not go with the CPU front-end (it needs --gpu-frontend): the CPU front-end's "
                                 "time interleaver is host state the file does not carry\n",
                         state_in.empty() ? "--state-out" : "--state-in");
            return 2;
        }

        InputFileReader reader;
        if (reader.Open(in_path, false) != 0) {
            std::fprintf(stderr, "dabmod_file: cannot read %s as an ETI file\n", in_path.c_str());
            return 1;
        }
        std::fprintf(stderr, "%s\n", reader.GetPrintableInfo().c_str());
        std::ofstream out(out_path, std::ios::binary);
        if (!out) {
            std::fprintf(stderr, "dabmod_file: cannot write %s\n", out_path.c_str());
            return 1;
        }

        std::unique_ptr<EtiFrontend> frontend;
        std::unique_ptr<DabGpuChain> chain;               // the one chain; with --contexts N: chain 0
        std::vector<std::unique_ptr<DabGpuChain>> more;   // --contexts N: chains 1 ... N - 1
        auto chain_of = [&](size_t j) -> DabGpuChain * { return j % contexts ? more[j % contexts - 1].get() : chain.get(); };
        size_t n_batches = 0, n_collected = 0, n_submitted = 0;     // batches queued / written, frames queued
        std::vector<uint8_t> leadin;              // --contexts N: the last frame of the batch queued last
        std::unique_ptr<FormatConverter> converter;
        Buffer bits, iq, converted;
        uint8_t frame[6144];
        size_t n_eti = 0, n_tf = 0, clipped = 0;
        std::vector<uint8_t> pending;             // --batch: hot-path input of the batch being filled
        std::deque<std::vector<uint8_t>> held;    // --batch with --reference-latency: the frames "inside the pipeline"
        size_t n_out = 0;                         // transmission frames written
        int in_flight = 0;
        DabGpuChain::MonitorTotals mon;           // --monitor: summed over the calls (and the contexts)
        auto add_monitor = [&](const DabGpuChain *ch) {
            if (!gs.monitor) return;
            const DabGpuChain::MonitorTotals &t = ch->monitor_totals();
            if (!t.frames) return;
            mon.worst_mer_db = mon.frames ? std::min(mon.worst_mer_db, t.worst_mer_db) : t.worst_mer_db;
            mon.frames += t.frames;
            mon.bit_errors += t.bit_errors;
            mon.n_bits += t.n_bits;
            mon.sum_mer_db += t.sum_mer_db;
        };
        // --dpd-feedback: the bytes just written against as many samples of RXFILE (short at its end: the common part)
        dabgpu_dpd_alignment dpd_al{};
        float dpd_peak = 0.f;
        bool dpd_aligned = false;
        std::vector<char> dpd_buf;
        auto dpd_feed = [&](DabGpuChain *ch, const void *p, size_t bytes) {
            if (!dpd) return;
            const int fmt = format == "s16" ? DABGPU_FMT_S16 : 0;
            size_t n = bytes / (fmt ? 4 : 8);
            dpd_buf.resize(n * 8);
            dpd_rx.read(dpd_buf.data(), static_cast<std::streamsize>(dpd_buf.size()));
            n = std::min(n, static_cast<size_t>(dpd_rx.gcount()) / 8);
            if (!n) return;
            auto chk = [&](int rc) { if (rc) throw std::runtime_error(std::string("--dpd-feedback: ") + dabgpu_last_error(ch->context())); };
            if (!dpd_aligned) {
                chk(dabgpu_dpd_align(ch->context(), p, fmt, dpd_buf.data(), n, &dpd_al));
                double peak2 = 0.0;
                for (size_t i = 0; i < n; ++i) {
                    const double re = fmt ? static_cast<const int16_t *>(p)[2 * i] : static_cast<const float *>(p)[2 * i];
                    const double im = fmt ? static_cast<const int16_t *>(p)[2 * i + 1] : static_cast<const float *>(p)[2 * i + 1];
                    peak2 = std::max(peak2, re * re + im * im);
                }
                dpd_peak = std::nextafter(static_cast<float>(std::sqrt(peak2)), INFINITY);     // (the largest sample lands in the last bin)
                dpd_aligned = true;
                std::fprintf(stderr, "dabmod_file: dpd: lag %d tau %.6f gain %.6f%+.6fj coherence %.6f peak %.6g\n", dpd_al.lag, dpd_al.tau,
                             dpd_al.gain_re, dpd_al.gain_im, dpd_al.coherence, static_cast<double>(dpd_peak));
            }
            chk(dabgpu_dpd_measure(ch->context(), p, fmt, dpd_buf.data(), n, &dpd_al, dpd_peak, dpd_bins, 1));
        };
        // --loopback: the ETI frames handed to the device that the decoder has not returned yet, oldest first (loop_first: the
        // stream index of the oldest; at most fifteen stay behind a batch), the decoder's position, and the totals
        std::deque<std::vector<uint8_t>> loop_eti;
        uint64_t loop_first = 0, loop_pos = 0;
        struct {
            unsigned long long frames = 0, fic_errors = 0, msc_errors = 0, n_bits = 0, corrected = 0, coded_bits = 0;
            unsigned long long metric = 0, soft_sum = 0, erasures = 0;      // --soft
        } loop;
        std::vector<uint8_t> loop_bits, loop_out, loop_ref;
        std::vector<int8_t> loop_soft;
        std::vector<uint8_t> loop_rx;             // --channel-cn: the batch behind the channel, in the output's format
        double channel_sigma = -1.0;              //   < 0: not installed yet (the first batch sets the level)
        int loop_early = -1;
        size_t loop_cifs = 1;
        // --blind: the receiving side's own context, and whether it has read its configuration yet
        struct RxContext {
            dabgpu_ctx *c = nullptr;
            ~RxContext() { if (c) dabgpu_destroy(c); }
        } rx;
        bool blind_configured = false;
        // --superframe: the sub-channel's place (read from the first frame's layout), the images carried over (four at the most),
        // and every candidate's record in stream order
        struct {
            size_t offset = 0, framesize = 0;
            std::vector<uint8_t> images, out;
            std::vector<dabgpu_sf_record> records;
        } sf;
        // --cir: the last batch, as written or (--loopback --channel-cn) as the channel emulator left it, and its chain
        std::vector<uint8_t> cir_last;
        DabGpuChain *cir_chain = nullptr;
        auto cir_keep = [&](DabGpuChain *ch, const void *p, size_t bytes) {
            if ((!cir && !carrier_mer) || bytes < ch->output_bytes_per_frame()) return;
            cir_last.assign(static_cast<const uint8_t *>(p), static_cast<const uint8_t *>(p) + bytes);
            cir_chain = ch;
        };
        auto loopback_batch = [&](DabGpuChain *ch, const void *p, size_t bytes) {
            dabgpu_ctx *c = ch->context();
            auto chk = [&](int rc) { if (rc) throw std::runtime_error(std::string("--loopback: ") + dabgpu_last_error(c)); };
            if (loop_early < 0) {
                // where --monitor puts the window: behind FIRFilter's look-ahead and the guard window's overlap
                loop_early = static_cast<int>(gs.ofdmWindowOverlap);
                for (RemoteControllable *rc : ch->remote_controllables())
                    if (rc->get_rc_name() == "firfilter") loop_early += std::stoi(rc->get_parameter("ntaps")) - 1;
            }
            const size_t n_frames = bytes / ch->output_bytes_per_frame(), n = n_frames * loop_cifs;
            const int loop_fmt = format == "s16" ? DABGPU_FMT_S16 : 0;
            if (channel) {
                dabgpu_geometry g{};
                chk(dabgpu_get_geometry(c, &g));
                if (channel_sigma < 0.0) {
                    const int reach = g.sym_size - g.spacing - loop_early;
                    for (const Echo &e : channel_echoes)
                        if (static_cast<long>(e.delay) > reach)
                            throw std::runtime_error("--channel-echo: a delay of " + std::to_string(e.delay) + " samples lies beyond the cyclic "
                                                     "prefix less the window's lead (" + std::to_string(reach) + "): that takes the synchroniser");
                    // mean power of the first batch's samples behind the null symbol
                    double sum = 0.0;
                    for (size_t f = 0; f < n_frames; ++f)
                        for (size_t i = static_cast<size_t>(g.null_size); i < g.tf_samples; ++i) {
                            const size_t at = 2 * (f * g.tf_samples + i);
                            const double re = loop_fmt ? static_cast<const int16_t *>(p)[at] : static_cast<const float *>(p)[at];
                            const double im = loop_fmt ? static_cast<const int16_t *>(p)[at + 1] : static_cast<const float *>(p)[at + 1];
                            sum += re * re + im * im;
                        }
                    const double power = sum / static_cast<double>(n_frames * (g.tf_samples - static_cast<size_t>(g.null_size)));
                    channel_sigma = std::sqrt(power / std::pow(10.0, channel_cn / 10.0) / 2.0);
                    dabgpu_channel_config cc{};
                    cc.n_paths = static_cast<uint32_t>(1 + channel_echoes.size());
                    cc.sigma = static_cast<float>(channel_sigma);
                    cc.seed = channel_seed;
                    cc.rate_hz = 2048000.0;
                    cc.paths[0].gain_re = 1.0f;
                    for (size_t k = 0; k < channel_echoes.size(); ++k) {
                        const Echo &e = channel_echoes[k];
                        const double amp = std::pow(10.0, e.db / 20.0);
                        cc.paths[k + 1].delay = e.delay;
                        cc.paths[k + 1].gain_re = static_cast<float>(amp * std::cos(e.phase));
                        cc.paths[k + 1].gain_im = static_cast<float>(amp * std::sin(e.phase));
                    }
                    chk(dabgpu_set_channel(c, &cc));
                    chk(dabgpu_channel_reset(c, 0));
                }
                loop_rx.resize(bytes);
                chk(dabgpu_channel(c, p, loop_fmt, n_frames * g.tf_samples, loop_rx.data(), loop_fmt));
                p = loop_rx.data();
                cir_keep(ch, p, bytes);
            }
            loop_bits.resize(n_frames * ch->input_bytes_per_frame());
            loop_out.resize(n * 6144);
            loop_ref.assign(n * 6144, 0);
            if (soft) {
                loop_soft.resize(8 * loop_bits.size());
                chk((csi ? dabgpu_demod_csi : dabgpu_demod_soft)(c, p, format == "s16" ? DABGPU_FMT_S16 : 0, n_frames, loop_early,
                                                                 loop_soft.data(), nullptr, nullptr));
            } else {
                chk(dabgpu_demod(c, p, format == "s16" ? DABGPU_FMT_S16 : 0, n_frames, loop_early, loop_bits.data(), nullptr));
            }
            dabgpu_ctx *dc = c;                       // the context that decodes
            if (blind) {
                if (!rx.c) {
                    dabgpu_geometry g{};
                    chk(dabgpu_get_geometry(c, &g));
                    const dabgpu_config rc{g.mode, 0, static_cast<int>(batch), 0};
                    uint8_t boot[6144];
                    if (dabgpu_create(&rc, &rx.c) || dabgpu_fic_bootstrap_frame(g.mode ? g.mode : 4, boot))
                        throw std::runtime_error(std::string("--blind: ") + dabgpu_last_error(nullptr));
                    if (dabgpu_frontend_configure(rx.c, boot)) throw std::runtime_error(std::string("--blind: ") + dabgpu_last_error(rx.c));
                }
                dc = rx.c;
            }
            auto chk_dc = [&](int rc) { if (rc) throw std::runtime_error(std::string("--loopback: ") + dabgpu_last_error(dc)); };
            if (blind && !blind_configured) {
                // the FIC alone, fifteen frames late; what it says; the decoder set up from it.  The batch is decoded again below.
                size_t ob0 = 0;
                chk_dc(dabgpu_decode(dc, loop_bits.data(), n_frames, loop_out.data(), loop_out.size(), nullptr, &ob0));
                chk_dc(dabgpu_fic_scan(dc, loop_out.data(), n, DABGPU_FIC_OFFSET_CONFIGURED));
                std::vector<dabgpu_fic_result> res(1);
                chk_dc(dabgpu_get_fic_result(dc, res.data()));
                const dabgpu_fic_result &r = res[0];
                std::fprintf(stderr, "dabmod_file: blind: %u FIBs: %u good, %u bad, %u zero; EId 0x%04X; %u sub-channels\n", r.fibs, r.fibs_ok,
                             r.fibs_bad, r.fibs_zero, r.eid, r.n_subch);
                for (uint32_t i = 0; i < r.n_subch && i < 64; ++i) {
                    const dabgpu_fic_subch &sc = r.sub[i];
                    std::fprintf(stderr, "dabmod_file: blind: SubChId %2u: start %3u CU, size %3u CU, %s, %3u kbit/s (TPL 0x%02X, STL %u)%s\n",
                                 sc.subchid, sc.sad, sc.size_cu,
                                 !sc.supported ? "not supported"
                                 : !sc.form    ? ("UEP " + std::to_string(sc.level)).c_str()
                                               : ("EEP " + std::to_string(sc.level) + (sc.index_option ? "-B" : "-A")).c_str(),
                                 sc.bitrate, sc.tpl, sc.stl, sc.changes ? ", redefined inside the batch" : "");
                }
                if (dabgpu_decode_configure_from_fic(dc)) throw BlindFailure(dabgpu_last_error(dc));
                std::vector<uint8_t> made(6144);
                if (dabgpu_fic_make_header(&r, static_cast<int>(gs.dabMode), made.data())) throw BlindFailure(dabgpu_last_error(nullptr));
                const std::vector<uint8_t> &sent = loop_eti.front();
                const size_t nst = sent[5] & 0x7fu;
                bool same = made[5] == sent[5] && ((made[6] ^ sent[6]) & 0x18) == 0;
                for (size_t k = 0; same && k < nst; ++k)                // (SAD, TPL, STL; the SCId is the SubChId here)
                    same = ((made[8 + 4 * k] ^ sent[8 + 4 * k]) & 3) == 0 && !std::memcmp(&made[9 + 4 * k], &sent[9 + 4 * k], 3);
                if (!same) throw BlindFailure("the FIC describes another layout than the file's STC words");
                blind_configured = true;
            }
            // output i is frame loop_pos + i - 15 of the stream
            for (size_t i = 0; i < n; ++i)
                if (loop_pos + i >= 15) std::memcpy(&loop_ref[i * 6144], loop_eti.at(loop_pos + i - 15 - loop_first).data(), 6144);
            size_t ob = 0;
            if (soft) chk(dabgpu_decode_soft(c, loop_soft.data(), n_frames, loop_out.data(), loop_out.size(), loop_ref.data(), &ob));
            else chk_dc(dabgpu_decode(dc, loop_bits.data(), n_frames, loop_out.data(), loop_out.size(), loop_ref.data(), &ob));
            for (size_t i = 0; i < n; ++i) {
                dabgpu_decode_stats all{}, fic{};
                if (soft) {
                    dabgpu_decode_soft_stats sa{}, sf{};
                    chk(dabgpu_get_decode_soft_stats(c, i, -1, &sa));
                    chk(dabgpu_get_decode_soft_stats(c, i, 0, &sf));
                    all.valid = sa.valid; all.corrected = sa.corrected; all.coded_bits = sa.coded_bits;
                    all.bit_errors = sa.bit_errors; all.n_bits = sa.n_bits;
                    fic.bit_errors = sf.bit_errors;
                    if (sa.valid) {
                        loop.metric += sa.metric;
                        loop.soft_sum += sa.soft_sum;
                        loop.erasures += sa.erasures;
                    }
                } else {
                    chk_dc(dabgpu_get_decode_stats(dc, i, -1, &all));
                    chk_dc(dabgpu_get_decode_stats(dc, i, 0, &fic));
                }
                if (!all.valid) continue;
                ++loop.frames;
                loop.fic_errors += fic.bit_errors;
                loop.msc_errors += all.bit_errors - fic.bit_errors;
                loop.n_bits += all.n_bits;
                loop.corrected += all.corrected;
                loop.coded_bits += all.coded_bits;
            }
            if (superframe >= 0) {
                if (!sf.framesize) {
                    std::vector<dabgpu_fe_layout> lay(1);
                    if (dabgpu_frontend_describe(loop_eti.front().data(), lay.data()))
                        throw std::runtime_error(std::string("--superframe: ") + dabgpu_last_error(nullptr));
                    if (static_cast<size_t>(superframe) >= lay[0].nst)
                        throw std::runtime_error("--superframe: the file has " + std::to_string(lay[0].nst) + " sub-channels");
                    sf.offset = lay[0].sub[superframe].offset;
                    sf.framesize = lay[0].sub[superframe].framesize;
                    if (dabgpu_superframe_check(5, sf.offset, sf.framesize))
                        throw std::runtime_error(std::string("--superframe: ") + dabgpu_last_error(nullptr));
                }
                for (size_t i = 0; i < n; ++i)
                    if (loop_pos + i >= 15) sf.images.insert(sf.images.end(), &loop_out[i * 6144], &loop_out[(i + 1) * 6144]);
                const size_t have = sf.images.size() / 6144;
                if (have >= 5) {
                    size_t ob = 0, got = 0;
                    sf.out.resize((have - 4) * 110 * (sf.framesize / 24));
                    chk_dc(dabgpu_superframe(dc, sf.images.data(), have, sf.offset, sf.framesize, sf.out.data(), sf.out.size(), &ob));
                    const size_t at = sf.records.size();
                    sf.records.resize(at + have - 4);
                    chk_dc(dabgpu_get_superframe_records(dc, &sf.records[at], have - 4, &got));
                    sf.images.erase(sf.images.begin(), sf.images.end() - 4 * 6144);
                }
            }
            loop_pos += n;
            while (loop_first + 15 < loop_pos) {
                loop_eti.pop_front();
                ++loop_first;
            }
        };
        // --tii-scan: the last batch of two frames or more, as written, and the chain it came from
        std::vector<uint8_t> tii_last;
        DabGpuChain *tii_chain = nullptr;
        auto tii_keep = [&](DabGpuChain *ch, const void *p, size_t bytes) {
            if (!tii_scan || bytes / ch->output_bytes_per_frame() < 2) return;
            tii_last.assign(static_cast<const uint8_t *>(p), static_cast<const uint8_t *>(p) + bytes);
            tii_chain = ch;
        };
        // the oldest batch in flight, in stream order: batch j lives on chain j mod N
        auto drain_one = [&]() {
            DabGpuChain *ch = chain_of(n_collected++);
            const void *p = nullptr;
            const size_t n = ch->collect(&p);
            add_monitor(ch);
            if (loopback) loopback_batch(ch, p, n);
            n_out += n / ch->output_bytes_per_frame();
            if (format != "complexf") clipped += ch->get_num_clipped_samples();
            out.write(static_cast<const char *>(p), static_cast<std::streamsize>(n));
            dpd_feed(ch, p, n);
            tii_keep(ch, p, n);
            if (!(loopback && channel)) cir_keep(ch, p, n);
            --in_flight;
        };
        // two batches in flight per chain; the owning chain starts from the state behind the frame before its batch
        auto submit_batch = [&](size_t frames) {
            if (in_flight == 2 * contexts) drain_one();
            DabGpuChain *ch = chain_of(n_batches++);
            if (contexts > 1) ch->seed(n_submitted ? leadin.data() : nullptr, n_submitted);
            ch->submit(pending.data(), frames);
            if (contexts > 1) leadin.assign(pending.begin() + (frames - 1) * ch->input_bytes_per_frame(),
                                            pending.begin() + frames * ch->input_bytes_per_frame());
            n_submitted += frames;
            ++in_flight;
        };
        // --gpu-frontend: the ETI frames of the batch being filled, and with --reference-latency the frames held back
        std::vector<uint8_t> pending_eti;
        std::deque<std::vector<uint8_t>> held_eti;
        size_t cifs = 1, n_gated = 0;             // ETI frames per transmission frame; frames since the one with FP = 0
        uint64_t n_before = 0;                    // --state-in: ETI frames the runs before this one modulated
        auto submit_eti_batch = [&](size_t frames) {
            if (in_flight == 2) drain_one();
            ++n_batches;
            chain->submit_eti(pending_eti.data(), frames * cifs);
            if (loopback) {
                loop_cifs = cifs;
                for (size_t k = 0; k < frames * cifs; ++k)
                    loop_eti.emplace_back(pending_eti.begin() + k * 6144, pending_eti.begin() + (k + 1) * 6144);
            }
            pending_eti.erase(pending_eti.begin(), pending_eti.begin() + frames * cifs * 6144);
            n_submitted += frames;
            ++in_flight;
        };
        for (int l = 0; l < loops; ++l) {
            if (l && reader.Open(in_path, false) != 0) return 1;
            int got;
            while ((got = reader.GetNextFrame(frame)) == 6144) {
                ++n_eti;
                if (gpu_frontend) {
                    if (!chain) {
                        // align the frame groups (src/DabMod.cpp:684-693); a continued stream is aligned where it was left
                        if (state_in.empty() && (frame[6] >> 5) != 0) continue;
                        if (gs.dabMode == 0) {
                            const unsigned mid = (frame[6] >> 3) & 3;
                            gs.dabMode = mid ? mid : 4;
                        }
                        cifs = gs.dabMode == 1 ? 4 : gs.dabMode == 4 ? 2 : 1;
                        if (!state_in.empty() && (frame[6] >> 5) % cifs) {
                            std::fprintf(stderr, "dabmod_file: --state-in: the first frame must open a transmission frame (FP = %u, "
                                                 "not a multiple of %zu)\n", unsigned(frame[6] >> 5), cifs);
                            return 1;
                        }
                        gs.outputFormat = format;
                        gs.maxBatchFrames = batch;
                        chain.reset(new DabGpuChain(gs));
                        chain->configure_frontend(frame);
                        if (!state_in.empty()) {
                            const StreamStateFile st = read_state(state_in);
                            chain->set_frontend_state(st.frontend);
                            chain->set_stream_state(st.chain);
                            n_before = st.n_eti;
                        }
                    }
                    if (++n_gated % cifs == 0) ++n_tf;
                    if (reference_latency) {
                        // transmission frame i is modulated when frame i + k is complete; the last k never are
                        held_eti.emplace_back(frame, frame + 6144);
                        if (held_eti.size() <= gs.referencePipelineDepth() * cifs) continue;
                        pending_eti.insert(pending_eti.end(), held_eti.front().begin(), held_eti.front().end());
                        held_eti.pop_front();
                    } else
                        pending_eti.insert(pending_eti.end(), frame, frame + 6144);
                    if (pending_eti.size() == batch * cifs * 6144) submit_eti_batch(batch);
                    continue;
                }
                if (!frontend) {
                    if (gs.dabMode == 0) {
                        // MID of the first frame; 0 means mode IV (EN 300 799 5.3.2)
                        const unsigned mid = (frame[6] >> 3) & 3;
                        gs.dabMode = mid ? mid : 4;
                    }
                    frontend.reset(new EtiFrontend(gs.dabMode));
                }
                if (!frontend->push(frame, bits)) continue;
                ++n_tf;
                if (bits_only) {
                    out.write(static_cast<const char *>(bits.getData()), static_cast<std::streamsize>(bits.getLength()));
                    continue;
                }
                if (batch > 1 && !separate_converter) {
                    // streaming shape: the front-end fills a batch while the GPU works on the previous two
                    if (!chain) {
                        gs.outputFormat = format;
                        gs.maxBatchFrames = batch;
                        chain.reset(new DabGpuChain(gs));
                        for (long k = 1; k < contexts; ++k) more.emplace_back(new DabGpuChain(gs));
                        pending.reserve(batch * bits.getLength());
                    }
                    const uint8_t *b = static_cast<const uint8_t *>(bits.getData());
                    if (reference_latency) {
                        // frame i is modulated when frame i + k has arrived; the last k frames never are (see --reference-latency)
                        held.emplace_back(b, b + bits.getLength());
                        if (held.size() <= gs.referencePipelineDepth()) continue;
                        pending.insert(pending.end(), held.front().begin(), held.front().end());
                        held.pop_front();
                    } else
                    pending.insert(pending.end(), b, b + bits.getLength());
                    if (pending.size() == batch * chain->input_bytes_per_frame()) {
                        submit_batch(batch);
                        pending.clear();
                    }
                    continue;
                }
                if (!chain) {
                    // the output format is the chain's own last step (stored by its last kernel for s16); the
                    // stand-alone FormatConverter plugin stays available with --separate-converter
                    if (!separate_converter) gs.outputFormat = format;
                    if (reference_latency) gs.emulatePipelineDrops = gs.referencePipelineDepth();
                    chain.reset(new DabGpuChain(gs));
                    if (separate_converter && format != "complexf") converter.reset(new FormatConverter(false, format));
                }
                if (chain->process(&bits, &iq) == 0) continue;       // (a frame inside the emulated pipeline: nothing yet)
                add_monitor(chain.get());
                ++n_out;
                const Buffer *o = &iq;
                if (converter) {
                    converter->process(&iq, &converted);
                    clipped += converter->get_num_clipped_samples();
                    o = &converted;
                } else if (format != "complexf") {
                    clipped += chain->get_num_clipped_samples();
                }
                out.write(static_cast<const char *>(o->getData()), static_cast<std::streamsize>(o->getLength()));
                dpd_feed(chain.get(), o->getData(), o->getLength());
                cir_keep(chain.get(), o->getData(), o->getLength());
            }
            if (got < 0) {
                std::fprintf(stderr, "dabmod_file: error while reading %s\n", in_path.c_str());
                return 1;
            }
        }
        if (chain && gpu_frontend) {
            // the tail: the whole transmission frames left over, then whatever is still in flight, in order
            const size_t rest = pending_eti.size() / (cifs * 6144);
            if (rest) submit_eti_batch(rest);
            while (in_flight) drain_one();
            if (!state_out.empty())
                write_state(state_out, {n_before + n_submitted * cifs, chain->frontend_state(), chain->get_stream_state()});
        } else if (chain && batch > 1 && !separate_converter) {
            // the tail: a last, shorter batch, then whatever is still in flight, in order
            const size_t rest = pending.size() / chain->input_bytes_per_frame();
            if (rest) submit_batch(rest);
            while (in_flight) drain_one();
        }
        if (gpu_frontend && !chain && !state_out.empty()) {
            std::fprintf(stderr, "dabmod_file: --state-out: no frame was modulated, there is no state to write\n");
            return 1;
        }
        if (bits_only) n_out = n_tf;
        std::fprintf(stderr, "dabmod_file: %zu ETI frames -> %zu transmission frames in, %zu out (mode %u)", n_eti, n_tf, n_out, gs.dabMode);
        if (format != "complexf") std::fprintf(stderr, ", %zu clipped components", clipped);
        std::fprintf(stderr, "\n");
        std::printf("%zu %zu %zu\n", n_eti, n_tf, n_out);
        if (gs.monitor) {
            std::fprintf(stderr, "dabmod_file: monitor: %zu frames decoded, %llu bit errors in %llu bits, MER worst %.2f dB, mean %.2f dB\n",
                         mon.frames, static_cast<unsigned long long>(mon.bit_errors), static_cast<unsigned long long>(mon.n_bits),
                         mon.worst_mer_db, mon.frames ? mon.sum_mer_db / static_cast<double>(mon.frames) : 0.0);
        }
        if (loopback) {
            std::fprintf(stderr, "dabmod_file: loopback: %llu frames compared, %llu FIC and %llu MSC payload bit errors in %llu bits, "
                                 "%llu corrected channel bits in %llu coded bits\n",
                         loop.frames, loop.fic_errors, loop.msc_errors, loop.n_bits, loop.corrected, loop.coded_bits);
            if (channel)
                std::fprintf(stderr, "dabmod_file: loopback: channel: C/N %.1f dB, seed %llu, %zu path%s, sigma %g\n", channel_cn, channel_seed,
                             1 + channel_echoes.size(), channel_echoes.empty() ? "" : "s", channel_sigma);
            if (soft)
                std::fprintf(stderr, "dabmod_file: loopback: soft decisions, metric %llu / soft_sum %llu, %llu erasures\n", loop.metric,
                             loop.soft_sum, loop.erasures);
        }
        unsigned long long sf_bad_aus = 0;
        if (superframe >= 0) {
            // the greedy walk of dabgpu_get_superframe_result, over the candidates of every batch
            unsigned long long found = 0, aus_ok = 0, corrected = 0, failed = 0;
            unsigned most = 0;
            long first = -1;
            for (size_t f = 0; f < sf.records.size();) {
                const dabgpu_sf_record &r = sf.records[f];
                if ((r.flags & (DABGPU_SF_FIRE_OK | DABGPU_SF_ZERO | DABGPU_SF_HEADER_VALID)) != (DABGPU_SF_FIRE_OK | DABGPU_SF_HEADER_VALID)) {
                    f += 1;
                    continue;
                }
                if (first < 0) first = static_cast<long>(f);
                const unsigned ok = static_cast<unsigned>(__builtin_popcount(r.au_ok));
                ++found;
                aus_ok += ok;
                sf_bad_aus += r.num_aus - ok;
                corrected += r.rs_corrected;
                failed += r.rs_failed;
                most = std::max<unsigned>(most, r.rs_max);
                f += 5;
            }
            std::fprintf(stderr, "dabmod_file: superframe: sub-channel %ld, %zu candidates, %llu superframes (first at %ld), AUs %llu ok / %llu bad, "
                                 "%llu RS bytes corrected (at most %u in a word), %llu words failed\n",
                         superframe, sf.records.size(), found, first, aus_ok, sf_bad_aus, corrected, most, failed);
        }
        int mask_violations = 0;
        if (gs.spectrum) {
            // the contexts' sums added: one spectrum of the whole file
            std::vector<double> raw(2048, 0.0);
            uint64_t segments = 0;
            double rate = 0.0;
            auto add = [&](DabGpuChain *ch) {
                const DabGpuChain::SpectrumTotals t = ch->spectrum_totals();
                if (!t.segments) return;
                for (size_t k = 0; k < raw.size(); ++k) raw[k] += t.raw[k];
                segments += t.segments;
                rate = t.rate_hz;
            };
            if (chain) add(chain.get());
            for (auto &m : more) add(m.get());
            if (!segments) {
                std::fprintf(stderr, "dabmod_file: --spectrum: nothing was modulated, there is no spectrum to write\n");
                return 1;
            }
            dabgpu_mask_result res;
            if (dabgpu_spectrum_check_mask(raw.data(), 2048, rate, mask_offs.data(), mask_limit.data(), static_cast<int>(mask_offs.size()),
                                           oob_from, &res) != 0)
                throw std::runtime_error(std::string("--spectrum: ") + dabgpu_last_error(nullptr));
            std::FILE *sf = std::fopen(spectrum_path.c_str(), "w");
            if (!sf) {
                std::fprintf(stderr, "dabmod_file: cannot write %s\n", spectrum_path.c_str());
                return 1;
            }
            for (int i = 0; i < 2048; ++i) {
                const int k = (i + 1024) & 2047;                       // ascending frequency: bins 1024 ... 2047, then 0 ... 1023
                std::fprintf(sf, "%.3f %.6f\n", static_cast<double>(k < 1024 ? k : k - 2048) * rate / 2048.0, 10.0 * std::log10(raw[k] / res.ref));
            }
            if (std::fclose(sf) != 0) {
                std::fprintf(stderr, "dabmod_file: cannot write %s\n", spectrum_path.c_str());
                return 1;
            }
            std::fprintf(stderr, "dabmod_file: spectrum: %llu segments at %.0f Hz, out-of-band maximum %.2f dB at %.0f Hz (from %.0f Hz)\n",
                         static_cast<unsigned long long>(segments), rate, res.oob_max_db, res.oob_freq_hz, oob_from);
            if (!mask_offs.empty()) {
                std::fprintf(stderr, "dabmod_file: mask: worst margin %.2f dB at %.0f Hz, %d of %d bins above the mask\n",
                             res.worst_margin_db, res.worst_freq_hz, res.n_violations, res.n_checked);
                mask_violations = res.n_violations;
            }
        }
        if (dpd) {
            if (!dpd_aligned) {
                std::fprintf(stderr, "dabmod_file: --dpd-feedback: nothing was measured (no output, or an empty feedback file)\n");
                return 1;
            }
            dabgpu_dpd_stats st;
            if (dabgpu_get_dpd_stats(chain->context(), &st) != 0)
                throw std::runtime_error(std::string("--dpd-feedback: ") + dabgpu_last_error(chain->context()));
            float am[5], pm[5];
            dabgpu_dpd_fit_info fi;
            if (dabgpu_dpd_fit_poly(&st, DABGPU_DPD_BASIS_MAGSQ, dpd_min_count, 1, 0.0, nullptr, nullptr, 1.0, 1.0, am, pm, &fi) != 0) {
                std::fprintf(stderr, "dabmod_file: dpd: the fit is refused: %s\n", dabgpu_last_error(nullptr));
                return 4;
            }
            // (FormatConverter's s16 is the complexf value truncated: amplitudes of s16 output are in the units of the stream the
            // predistorter runs on, so the coefficients hold for either format)
            std::FILE *cf = std::fopen(dpd_out_path.c_str(), "w");
            if (!cf) {
                std::fprintf(stderr, "dabmod_file: cannot write %s\n", dpd_out_path.c_str());
                return 1;
            }
            std::fprintf(cf, "1\n5\n");
            for (int i = 0; i < 5; ++i) std::fprintf(cf, "%.9g\n", static_cast<double>(am[i]));
            for (int i = 0; i < 5; ++i) std::fprintf(cf, "%.9g\n", static_cast<double>(pm[i]));
            if (std::fclose(cf) != 0) {
                std::fprintf(stderr, "dabmod_file: cannot write %s\n", dpd_out_path.c_str());
                return 1;
            }
            std::fprintf(stderr, "dabmod_file: dpd: %llu samples in %d bins (%llu above the peak), %d bins fitted, residual am %.3g pm %.3g -> %s\n",
                         static_cast<unsigned long long>(st.samples_used), st.n_bins, static_cast<unsigned long long>(st.overflow),
                         fi.bins_used, fi.resid_am, fi.resid_pm, dpd_out_path.c_str());
        }
        bool tii_mismatch = false;
        if (tii_scan) {
            if (!tii_chain) {
                std::fprintf(stderr, "dabmod_file: --tii-scan: no batch of two frames or more was written, there is nothing to scan\n");
                return 1;
            }
            dabgpu_ctx *c = tii_chain->context();
            dabgpu_tii_scan_config cfg{};
            cfg.early = static_cast<int>(gs.ofdmWindowOverlap);           // where --monitor puts the window
            for (RemoteControllable *rc : tii_chain->remote_controllables())
                if (rc->get_rc_name() == "firfilter") cfg.early += std::stoi(rc->get_parameter("ntaps")) - 1;
            cfg.old_variant = gs.tiiConfig.old_variant ? 1 : 0;
            cfg.min_ratio = 12.0f;
            cfg.min_rel = 1e-3f;
            const size_t n_frames = tii_last.size() / tii_chain->output_bytes_per_frame();
            dabgpu_tii_scan_head head;
            dabgpu_tii_entry ent[24];
            if (dabgpu_tii_scan(c, tii_last.data(), format == "s16" ? DABGPU_FMT_S16 : 0, n_frames, &cfg) != 0 ||
                dabgpu_get_tii_scan(c, &head, ent, 24) != 0)
                throw std::runtime_error(std::string("--tii-scan: ") + dabgpu_last_error(c));
            std::fprintf(stderr, "dabmod_file: tii: %zu frames scanned, %d used (parity %d), window %d samples early, floor %.3g, %d entr%s\n",
                         n_frames, head.n_used, head.parity, cfg.early, head.floor, head.n_entries, head.n_entries == 1 ? "y" : "ies");
            for (int i = 0; i < head.n_entries && i < 24; ++i)
                std::fprintf(stderr, "dabmod_file: tii: comb %d pattern %d mask 0x%02x (%d cells) level %.2f dB delay %+.3f samples "
                                     "(coarse %+.2f, runner-up %.3f)\n", ent[i].comb, ent[i].pattern, ent[i].mask, ent[i].n_set,
                             10.0 * std::log10(ent[i].energy), ent[i].delay, ent[i].delay_coarse, ent[i].runner_up);
            if (gs.tiiConfig.enable) {
                // the pattern as the standard reads it: row p of the words of weight four, in Mode II with its halves exchanged
                int word = 0, want = -1;
                for (int w = 0, idx = 0; w < 256; ++w)
                    if (__builtin_popcount(static_cast<unsigned>(w)) == 4 && idx++ == gs.tiiConfig.pattern) word = w;
                if (gs.dabMode == 2) word = ((word & 0x0f) << 4) | (word >> 4);
                for (int w = 0, idx = 0; w <= word; ++w)
                    if (__builtin_popcount(static_cast<unsigned>(w)) == 4) want = idx++;
                tii_mismatch = head.n_entries != 1 || ent[0].comb != gs.tiiConfig.comb || ent[0].pattern != want;
                std::fprintf(stderr, "dabmod_file: tii: configured comb %d pattern %d, read by the standard as pattern %d: %s\n",
                             gs.tiiConfig.comb, gs.tiiConfig.pattern, want, tii_mismatch ? "NOT what was read" : "read");
            }
        }
        if (cir) {
            if (!cir_chain) {
                std::fprintf(stderr, "dabmod_file: --cir: no frame was written, there is nothing to measure\n");
                return 1;
            }
            dabgpu_ctx *c = cir_chain->context();
            dabgpu_geometry g{};
            dabgpu_cir_config cfg{};
            cfg.early = static_cast<int>(gs.ofdmWindowOverlap);           // where --monitor puts the window
            for (RemoteControllable *rc : cir_chain->remote_controllables())
                if (rc->get_rc_name() == "firfilter") cfg.early += std::stoi(rc->get_parameter("ntaps")) - 1;
            cfg.window = 1;
            cfg.min_ratio = 20.0f;
            cfg.min_rel = 1e-3f;
            const size_t n_frames = cir_last.size() / cir_chain->output_bytes_per_frame();
            dabgpu_cir_head head;
            dabgpu_cir_path path[DABGPU_CIR_MAX_PATHS];
            if (dabgpu_get_geometry(c, &g) != 0 ||
                dabgpu_cir(c, cir_last.data(), format == "s16" ? DABGPU_FMT_S16 : 0, n_frames, &cfg) != 0 ||
                dabgpu_get_cir(c, &head, path, DABGPU_CIR_MAX_PATHS) != 0)
                throw std::runtime_error(std::string("--cir: ") + dabgpu_last_error(c));
            std::vector<double> pdp(static_cast<size_t>(g.spacing));
            if (dabgpu_get_cir_profile(c, pdp.data(), nullptr) != 0) throw std::runtime_error(std::string("--cir: ") + dabgpu_last_error(c));
            std::fprintf(stderr, "dabmod_file: cir: %zu frames%s, window %d samples early, floor %.1f dB below the peak, %d peak%s, %d path%s, "
                                 "mean delay %+.2f, delay spread %.2f samples, %.4f of the paths' power beyond the guard interval\n",
                         n_frames, loopback && channel ? " behind the channel" : "", cfg.early,
                         head.peak > 0.0 && head.floor > 0.0 ? 10.0 * std::log10(head.peak / head.floor) : 0.0, head.n_peaks,
                         head.n_peaks == 1 ? "" : "s", head.n_paths, head.n_paths == 1 ? "" : "s", head.mean_delay, head.delay_spread,
                         head.outside_guard);
            for (int i = 0; i < head.n_paths && i < DABGPU_CIR_MAX_PATHS; ++i)
                std::fprintf(stderr, "dabmod_file: cir: path delay %+.0f samples level %.2f dB fine %+.3f\n", path[i].delay,
                             10.0 * std::log10(path[i].power / path[0].power), path[i].fine);
            std::FILE *cf = std::fopen(cir_path.c_str(), "w");
            if (!cf) {
                std::fprintf(stderr, "dabmod_file: cannot write %s\n", cir_path.c_str());
                return 1;
            }
            // one line per tap in ascending delay: taps N/2 ... N - 1 lie before tap 0
            const int N = g.spacing;
            for (int i = 0; i < N; ++i) {
                const int l = (i + N / 2) % N;
                const double level = head.peak > 0.0 && pdp[static_cast<size_t>(l)] > 0.0
                                         ? 10.0 * std::log10(pdp[static_cast<size_t>(l)] / head.peak) : -400.0;
                std::fprintf(cf, "%d %.3f\n", (l < N / 2 ? l : l - N) - cfg.early, level);
            }
            if (std::fclose(cf) != 0) {
                std::fprintf(stderr, "dabmod_file: cannot write %s\n", cir_path.c_str());
                return 1;
            }
        }
        if (carrier_mer) {
            if (!cir_chain) {
                std::fprintf(stderr, "dabmod_file: --carrier-mer: no frame was written, there is nothing to measure\n");
                return 1;
            }
            dabgpu_ctx *c = cir_chain->context();
            dabgpu_geometry g{};
            int early = static_cast<int>(gs.ofdmWindowOverlap);           // where --monitor puts the window
            for (RemoteControllable *rc : cir_chain->remote_controllables())
                if (rc->get_rc_name() == "firfilter") early += std::stoi(rc->get_parameter("ntaps")) - 1;
            const size_t n_frames = cir_last.size() / cir_chain->output_bytes_per_frame();
            if (dabgpu_get_geometry(c, &g) != 0 ||
                dabgpu_demod_carrier_state(c, cir_last.data(), format == "s16" ? DABGPU_FMT_S16 : 0, n_frames, early) != 0)
                throw std::runtime_error(std::string("--carrier-mer: ") + dabgpu_last_error(c));
            std::FILE *mf = std::fopen(carrier_mer_path.c_str(), "w");
            if (!mf) {
                std::fprintf(stderr, "dabmod_file: cannot write %s\n", carrier_mer_path.c_str());
                return 1;
            }
            const size_t K = static_cast<size_t>(g.carriers);
            std::vector<int64_t> A(K), V(K);
            std::vector<float> w(K);
            std::vector<double> all;
            const double scale = std::ldexp(1.0, DABGPU_CSI_FRAC_BITS - 1) * static_cast<double>(g.nb_symbols - 1);
            for (size_t f = 0; f < n_frames; ++f) {
                if (dabgpu_get_carrier_state(c, f, A.data(), V.data(), w.data()) != 0)
                    throw std::runtime_error(std::string("--carrier-mer: ") + dabgpu_last_error(c));
                for (size_t k = 0; k < K; ++k) {
                    const double mer = V[k] > 0 && A[k] > 0 ? 20.0 * std::log10(static_cast<double>(A[k]) / std::sqrt(scale * static_cast<double>(V[k])))
                                       : A[k] > 0 ? 400.0 : -400.0;
                    all.push_back(mer);
                    std::fprintf(mf, "%zu %zu %.3f %.6f\n", f, k, mer, static_cast<double>(w[k]));
                }
            }
            if (std::fclose(mf) != 0) {
                std::fprintf(stderr, "dabmod_file: cannot write %s\n", carrier_mer_path.c_str());
                return 1;
            }
            std::sort(all.begin(), all.end());
            std::fprintf(stderr, "dabmod_file: carrier-mer: %zu frames%s, window %d samples early, %zu carriers: median %.2f dB, lowest %.2f dB\n",
                         n_frames, loopback && channel ? " behind the channel" : "", early, K, all[all.size() / 2], all.front());
        }
        if (gs.monitor && mon.bit_errors) return 2;
        if (superframe >= 0) {
            if (sf_bad_aus) return 2;
        } else if (loopback && (loop.fic_errors || loop.msc_errors)) return 2;
        if (tii_mismatch) return 2;
        if (mask_violations) return 3;
        return 0;
    } catch (const BlindFailure &e) {
        std::fprintf(stderr, "dabmod_file: blind: no configuration could be read: %s\n", e.what());
        return 4;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "dabmod_file: %s\n", e.what());
        return 1;
    }
}
