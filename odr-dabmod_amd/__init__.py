"""odr-dabmod_amd -- MI355X-native DAB COFDM hot path.

Python plumbing over the C-ABI of include/dabgpu.h (libdabgpu.so: hand-written
gfx950 HIP kernels).  PyTorch is used only for device memory, streams and
torch.distributed; all arithmetic happens in the HIP library.  There is no CPU
fallback: if the library or a gfx950 device is missing, construction raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_DIR, "csrc")
# DABGPU_LIB selects another build of the same library (tuning sweeps); never a fallback
LIB_PATH = os.environ.get("DABGPU_LIB") or os.path.join(_CSRC, "libdabgpu.so")

STAGE_GAIN, STAGE_FIR, STAGE_RESAMPLE, STAGE_POLY, STAGE_NOGUARD = 1, 2, 4, 8, 1 << 8
GAIN_FIX, GAIN_MAX, GAIN_VAR = 0, 1, 2

EXPORTS = [
    "dabgpu_create", "dabgpu_destroy", "dabgpu_last_error", "dabgpu_version", "dabgpu_get_geometry",
    "dabgpu_set_gain", "dabgpu_set_fir_taps", "dabgpu_set_fir_default_taps",
    "dabgpu_set_window_overlap", "dabgpu_set_resampler", "dabgpu_set_poly", "dabgpu_set_lut",
    "dabgpu_qpsk_process", "dabgpu_freq_interleave_process", "dabgpu_phase_reference_process",
    "dabgpu_diff_mod_process", "dabgpu_null_symbol_process", "dabgpu_signal_mux_process",
    "dabgpu_ofdm_process", "dabgpu_gain_process", "dabgpu_guard_process", "dabgpu_fir_process",
    "dabgpu_resampler_process", "dabgpu_poly_process", "dabgpu_chain_out_bytes_per_frame",
    "dabgpu_chain_process", "dabgpu_chain_process_dev", "dabgpu_symbols_process_dev",
    "dabgpu_synchronize",
    "dabgpu_chain_submit", "dabgpu_chain_collect", "dabgpu_set_cfr", "dabgpu_get_cfr_stats",
    "dabgpu_cic_equalizer_process", "dabgpu_set_tii", "dabgpu_tii_process",
    "dabgpu_format_size", "dabgpu_format_process", "dabgpu_format_process_dev",
    "dabgpu_set_output_format", "dabgpu_get_num_clipped", "dabgpu_fir_inverse_design",
    "dabgpu_set_fir_boundary_mode", "dabgpu_debug_last_variant", "dabgpu_debug_trace",
    "dabgpu_set_lanes", "dabgpu_wait_for_stream", "dabgpu_stream_wait_for", "dabgpu_set_handover_frames",
    "dabgpu_post_process_dev", "dabgpu_debug_lanes", "dabgpu_set_gain_rounding",
    "dabgpu_stream_state_bytes", "dabgpu_get_stream_state", "dabgpu_set_stream_state",
    "dabgpu_chain_seed", "dabgpu_chain_seed_dev",
    "dabgpu_frontend_describe", "dabgpu_frontend_configure", "dabgpu_frontend_reset", "dabgpu_frontend_process",
    "dabgpu_frontend_process_dev", "dabgpu_chain_process_eti", "dabgpu_chain_submit_eti",
    "dabgpu_frontend_state_bytes", "dabgpu_frontend_get_state", "dabgpu_frontend_set_state",
    "dabgpu_frontend_seed", "dabgpu_frontend_seed_dev", "dabgpu_chain_seed_eti", "dabgpu_chain_seed_eti_dev",
    "dabgpu_set_cic_equalizer", "dabgpu_carriers_process", "dabgpu_carriers_process_dev",
    "dabgpu_demod", "dabgpu_demod_dev", "dabgpu_get_demod_stats", "dabgpu_demod_check_early", "dabgpu_set_monitor",
    "dabgpu_debug_demod_run_symbols",
    "dabgpu_spectrum_window", "dabgpu_spectrum", "dabgpu_spectrum_dev", "dabgpu_get_spectrum", "dabgpu_reset_spectrum",
    "dabgpu_set_spectrum_monitor", "dabgpu_debug_spectrum_run_segments", "dabgpu_spectrum_check_mask",
    "dabgpu_dpd_xspectrum", "dabgpu_dpd_xspectrum_dev", "dabgpu_get_dpd_xspectrum", "dabgpu_dpd_solve_alignment",
    "dabgpu_dpd_align", "dabgpu_dpd_align_dev", "dabgpu_dpd_delay_taps", "dabgpu_dpd_measure", "dabgpu_dpd_measure_dev",
    "dabgpu_get_dpd_stats", "dabgpu_reset_dpd", "dabgpu_debug_dpd_run_segments", "dabgpu_debug_dpd_tile",
    "dabgpu_dpd_fit_poly", "dabgpu_debug_resampler_run_hops", "dabgpu_debug_resampler_last_launch",
    "dabgpu_decode_check_layout", "dabgpu_decode_reset", "dabgpu_decode_dev", "dabgpu_decode", "dabgpu_get_decode_stats",
    "dabgpu_demod_soft", "dabgpu_demod_soft_dev", "dabgpu_decode_soft", "dabgpu_decode_soft_dev", "dabgpu_get_decode_soft_stats",
    "dabgpu_sync_dev", "dabgpu_sync", "dabgpu_get_sync_result", "dabgpu_sync_extract_dev", "dabgpu_sync_extract", "dabgpu_sync_check",
    "dabgpu_channel_check", "dabgpu_set_channel", "dabgpu_channel_reset", "dabgpu_get_channel_position", "dabgpu_channel_dev",
    "dabgpu_channel", "dabgpu_debug_channel_run_samples",
    "dabgpu_clock_check", "dabgpu_clock_step", "dabgpu_clock_count", "dabgpu_clock_out_max", "dabgpu_clock_phase_taps",
    "dabgpu_clock_inverse_ppm", "dabgpu_set_clock", "dabgpu_clock_reset", "dabgpu_get_clock_position", "dabgpu_clock_dev",
    "dabgpu_clock", "dabgpu_debug_clock_run_samples", "dabgpu_sco_dev", "dabgpu_sco", "dabgpu_get_sco",
    "dabgpu_tuner_check", "dabgpu_tuner_geometry", "dabgpu_tuner_taps", "dabgpu_tuner_count", "dabgpu_tuner_out_max",
    "dabgpu_set_tuner", "dabgpu_tuner_reset", "dabgpu_get_tuner_position", "dabgpu_tuner_dev", "dabgpu_tuner",
    "dabgpu_debug_tuner_run_samples",
    "dabgpu_tii_scan_dev", "dabgpu_tii_scan", "dabgpu_get_tii_scan", "dabgpu_tii_scan_check",
    "dabgpu_cir_dev", "dabgpu_cir", "dabgpu_get_cir", "dabgpu_get_cir_profile", "dabgpu_cir_check",
    "dabgpu_demod_csi", "dabgpu_demod_csi_dev", "dabgpu_demod_carrier_state", "dabgpu_demod_carrier_state_dev",
    "dabgpu_get_carrier_state", "dabgpu_debug_csi_unit_weights",
    "dabgpu_fic_scan_dev", "dabgpu_fic_scan", "dabgpu_get_fic_result", "dabgpu_get_fic_records", "dabgpu_get_fic_services",
    "dabgpu_fic_bootstrap_frame", "dabgpu_fic_make_header", "dabgpu_decode_configure_from_fic",
    "dabgpu_superframe_dev", "dabgpu_superframe", "dabgpu_get_superframe_result", "dabgpu_get_superframe_records",
    "dabgpu_superframe_check",
]

FORMATS = {"s16": (1, np.int16), "u8": (2, np.uint8), "s8": (3, np.int8)}


class DabGpuError(RuntimeError):
    pass


def source_hash():
    """SHA-256 (first 16 hex digits) over the sources libdabgpu.so is built from: ties a set of profiler counters
    (profiles/traffic.json) to the kernels they were collected on."""
    import hashlib
    h = hashlib.sha256()
    names = sorted(n for n in os.listdir(_CSRC) if n.endswith((".hip", ".h")) or n == "Makefile")
    for name in names:
        h.update(name.encode())
        h.update(open(os.path.join(_CSRC, name), "rb").read())
    h.update(open(os.path.join(os.path.dirname(_CSRC), "..", "include", "dabgpu.h"), "rb").read())
    return h.hexdigest()[:16]


def build(verbose=False):
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", _CSRC, "-j%d" % max(2, min(8, os.cpu_count() or 2))]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return LIB_PATH


class _Config(C.Structure):
    _fields_ = [("mode", C.c_int), ("device", C.c_int), ("max_frames", C.c_int),
                ("chunks_per_frame", C.c_int)]


class _CfrStats(C.Structure):
    _fields_ = [("num_clip", C.c_uint64), ("num_error_clip", C.c_uint64), ("num_samples", C.c_uint64),
                ("mer_symbol", C.c_int), ("mer_sum_iq", C.c_double), ("mer_sum_delta", C.c_double),
                ("nb_symbols", C.c_int), ("papr_before", C.c_double * 2 * 154), ("papr_after", C.c_double * 2 * 154)]


class _DemodStats(C.Structure):
    _fields_ = [("sum_signal", C.c_double), ("sum_quadrature", C.c_double), ("bit_errors", C.c_uint64),
                ("n_bits", C.c_uint64), ("min_margin", C.c_double)]


class _ScoFrame(C.Structure):
    _fields_ = [("a_hi_re", C.c_double), ("a_hi_im", C.c_double), ("a_lo_re", C.c_double), ("a_lo_im", C.c_double),
                ("s", C.c_double), ("ppm", C.c_double), ("residual_cfo", C.c_double), ("quality", C.c_double),
                ("valid", C.c_int32), ("reserved", C.c_int32)]


class _SyncFrame(C.Structure):
    _fields_ = [("start", C.c_int64), ("shift", C.c_int), ("valid", C.c_int), ("eps", C.c_double), ("cfo_hz", C.c_double),
                ("quality", C.c_double), ("null_depth", C.c_double)]


class _TiiScanConfig(C.Structure):
    _fields_ = [("early", C.c_int), ("old_variant", C.c_int), ("min_ratio", C.c_float), ("min_rel", C.c_float)]


class _TiiScanHead(C.Structure):
    _fields_ = [("n_used", C.c_int), ("parity", C.c_int), ("n_entries", C.c_int), ("reserved", C.c_int),
                ("floor", C.c_double), ("total", C.c_double * 2)]


class _TiiEntry(C.Structure):
    _fields_ = [("comb", C.c_int), ("pattern", C.c_int), ("mask", C.c_int), ("n_set", C.c_int), ("energy", C.c_double),
                ("delay_coarse", C.c_double), ("delay", C.c_double), ("runner_up", C.c_double)]


TII_SLOTS = 24


class _CirConfig(C.Structure):
    _fields_ = [("early", C.c_int), ("window", C.c_int), ("min_ratio", C.c_float), ("min_rel", C.c_float)]


class _CirHead(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("n_frames", "n_peaks", "n_paths", "window", "peak_index", "resp_min_bin", "resp_max_bin",
                                       "reserved")] + \
               [(k, C.c_double) for k in ("floor", "threshold", "peak", "total", "path_power", "mean_delay", "delay_spread",
                                          "first_delay", "outside_guard", "resp_mean", "resp_min", "resp_max")]


class _CirPath(C.Structure):
    _fields_ = [("index", C.c_int), ("reserved", C.c_int), ("delay", C.c_double), ("fine", C.c_double), ("power", C.c_double)]


CIR_MAX_PATHS = 16
CSI_FRAC_BITS, CSI_MAX_WEIGHT = 16, 4
CIR_RECTANGULAR, CIR_HANN = 0, 1
CH_MAX_PATHS, CH_MAX_DELAY = 64, 2047


class _ChannelPath(C.Structure):
    _fields_ = [("delay", C.c_uint32), ("gain_re", C.c_float), ("gain_im", C.c_float), ("doppler_hz", C.c_double)]


class _ChannelConfig(C.Structure):
    _fields_ = [("n_paths", C.c_uint32), ("sigma", C.c_float), ("seed", C.c_uint64), ("rate_hz", C.c_double),
                ("paths", _ChannelPath * CH_MAX_PATHS)]


class _TunerConfig(C.Structure):
    _fields_ = [("in_rate_hz", C.c_uint32), ("selectivity", C.c_int), ("offset_hz", C.c_double)]


class _DecodeSoftStats(C.Structure):
    _fields_ = [("valid", C.c_uint32), ("metric", C.c_uint64), ("contra_sum", C.c_uint64), ("soft_sum", C.c_uint64),
                ("corrected", C.c_uint64), ("erasures", C.c_uint64), ("coded_bits", C.c_uint64), ("bit_errors", C.c_uint64),
                ("n_bits", C.c_uint64)]


class _DecodeStats(C.Structure):
    _fields_ = [("valid", C.c_uint32), ("corrected", C.c_uint64), ("coded_bits", C.c_uint64), ("bit_errors", C.c_uint64),
                ("n_bits", C.c_uint64)]


class _SpectrumInfo(C.Structure):
    _fields_ = [("segments", C.c_uint64), ("nfft", C.c_int), ("window", C.c_int), ("sum_w2", C.c_double),
                ("rate_hz", C.c_double)]


class _MaskResult(C.Structure):
    _fields_ = [("ref", C.c_double), ("worst_margin_db", C.c_double), ("worst_freq_hz", C.c_double),
                ("n_violations", C.c_int), ("n_checked", C.c_int), ("oob_max_db", C.c_double), ("oob_freq_hz", C.c_double)]


class _DpdAlignment(C.Structure):
    _fields_ = [("lag", C.c_int), ("tau", C.c_double), ("gain_re", C.c_double), ("gain_im", C.c_double),
                ("coherence", C.c_double)]


DPD_MAX_BINS, DPD_MAX_LAG, DPD_TAPS = 256, 1000, 32
DPD_BASIS = {"magsq": 0, "reference": 1}


class _DpdStats(C.Structure):
    _fields_ = [("n_bins", C.c_int), ("peak", C.c_float), ("overflow", C.c_uint64), ("samples_used", C.c_uint64),
                ("count", C.c_uint64 * DPD_MAX_BINS), ("sum_tx", C.c_double * DPD_MAX_BINS),
                ("sum_rx", C.c_double * DPD_MAX_BINS), ("sum_phase", C.c_double * DPD_MAX_BINS),
                ("sum_rx2", C.c_double * DPD_MAX_BINS), ("sum_phase2", C.c_double * DPD_MAX_BINS),
                ("raw", C.c_int64 * 6 * DPD_MAX_BINS)]


class _DpdFitInfo(C.Structure):
    _fields_ = [("bins_used", C.c_int), ("cond_am", C.c_double), ("cond_pm", C.c_double), ("resid_am", C.c_double),
                ("resid_pm", C.c_double)]


SPECTRUM_NFFT = 2048
WINDOWS = {"rect": 0, "hann": 1, "blackman-harris": 2}
OOB_FROM_HZ = 970e3                                # where callers start to look for the out-of-band maximum by default


class _Geometry(C.Structure):
    _fields_ = [("mode", C.c_int), ("nb_symbols", C.c_int), ("carriers", C.c_int),
                ("spacing", C.c_int), ("null_size", C.c_int), ("sym_size", C.c_int),
                ("tf_input_bytes", C.c_size_t), ("tf_samples", C.c_size_t)]


class _FeRule(C.Structure):
    _fields_ = [("groups", C.c_uint32), ("pattern", C.c_uint32)]


class _FeSubch(C.Structure):
    _fields_ = [("sad", C.c_uint32), ("stl", C.c_uint32), ("tpl", C.c_uint32), ("framesize", C.c_uint32),
                ("cu", C.c_uint32), ("padding_byte", C.c_uint32), ("offset", C.c_uint32), ("n_rules", C.c_uint32),
                ("rule", _FeRule * 4)]


class _FeLayout(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("fic_bytes", C.c_uint32), ("fic_offset", C.c_uint32), ("fic_n_rules", C.c_uint32),
                ("fic_rule", _FeRule * 4), ("tail_bytes", C.c_uint32), ("tail_pattern", C.c_uint32), ("nst", C.c_uint32),
                ("sub", _FeSubch * 127)]


class _FicSubEntry(C.Structure):
    _fields_ = [("raw", C.c_uint32), ("sad", C.c_uint16), ("size", C.c_uint16), ("subchid", C.c_uint8), ("form", C.c_uint8),
                ("sw_option", C.c_uint8), ("index_level", C.c_uint8)]


class _FicServiceEntry(C.Structure):
    _fields_ = [("sid", C.c_uint16), ("info", C.c_uint8), ("first_comp", C.c_uint8)]


class _FicComponent(C.Structure):
    _fields_ = [("id", C.c_uint16), ("tmid", C.c_uint8), ("type", C.c_uint8), ("primary", C.c_uint8), ("ca", C.c_uint8),
                ("service", C.c_uint8), ("reserved", C.c_uint8)]


class _FicLabel(C.Structure):
    _fields_ = [("kind", C.c_uint8), ("charset", C.c_uint8), ("id", C.c_uint16), ("flag", C.c_uint16), ("text", C.c_uint8 * 16),
                ("reserved", C.c_uint16)]


class _FicRecord(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("eid_first", C.c_uint16), ("eid", C.c_uint16), ("eid_seen", C.c_uint8),
                ("eid_changes", C.c_uint8), ("change", C.c_uint8), ("alarm", C.c_uint8), ("cif_hi", C.c_uint8),
                ("cif_lo", C.c_uint8), ("n_sub", C.c_uint8), ("n_svc", C.c_uint8), ("n_comp", C.c_uint8),
                ("services_dropped", C.c_uint8), ("components_dropped", C.c_uint8), ("labels_dropped", C.c_uint8),
                ("figs_truncated", C.c_uint8), ("fig0_skipped", C.c_uint8), ("reserved", C.c_uint8 * 2),
                ("figs_type", C.c_uint8 * 8), ("fig0_ext", C.c_uint8 * 32), ("sub", _FicSubEntry * 9),
                ("svc", _FicServiceEntry * 4), ("comp", _FicComponent * 8), ("label", _FicLabel), ("pad", C.c_uint8 * 12)]


_FIC_SUBCH_FIELDS = ("subchid", "sad", "size_cu", "form", "index_option", "level", "bitrate", "tpl", "stl", "supported", "seen",
                     "changes", "first_fib", "last_fib", "raw", "table_switch")
_FIC_RESULT_FIELDS = ("fibs", "fibs_ok", "fibs_bad", "fibs_zero", "figs_truncated", "fig0_skipped", "services_dropped",
                      "components_dropped", "labels_dropped", "eid", "eid_seen", "eid_changes", "eid_first_fib", "eid_last_fib",
                      "n_subch", "reserved")


class _FicSubch(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in _FIC_SUBCH_FIELDS]


class _FicResult(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in _FIC_RESULT_FIELDS] + [("figs_type", C.c_uint32 * 8), ("fig0_ext", C.c_uint32 * 32),
                                                                 ("sub", _FicSubch * 64)]


class _FicService(C.Structure):
    _fields_ = [("sid", C.c_uint32), ("n_components", C.c_uint32), ("sightings", C.c_uint32), ("components_dropped", C.c_uint32),
                ("comp", _FicComponent * 12), ("label", _FicLabel)]


assert C.sizeof(_FicRecord) == 288 and C.sizeof(_FicResult) == 4320 and C.sizeof(_FicService) == 136
FIC_RECORD_BYTES, FIC_OFFSET_CONFIGURED = 288, C.c_size_t(-1).value
FIC_CRC_OK, FIC_ZERO, FIC_TRUNCATED = 1, 2, 4


class _SfRecord(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("rs_corrected", C.c_uint16), ("rs_failed", C.c_uint16), ("rs_max", C.c_uint8),
                ("num_aus", C.c_uint8), ("au_ok", C.c_uint8), ("header", C.c_uint8), ("rfa", C.c_uint8), ("dac_rate", C.c_uint8),
                ("sbr_flag", C.c_uint8), ("aac_channel_mode", C.c_uint8), ("ps_flag", C.c_uint8), ("mpeg_surround_config", C.c_uint8),
                ("reserved0", C.c_uint8 * 2), ("au_start", C.c_uint16 * 7), ("fire_crc", C.c_uint16), ("cw_errors", C.c_uint8 * 24),
                ("reserved1", C.c_uint32)]


_SF_RESULT_FIELDS = ("candidates", "superframes", "first", "phase_changes", "aus", "aus_ok", "aus_bad", "rs_failed", "rs_max",
                     "reserved", "rs_corrected")


class _SfResult(C.Structure):
    _fields_ = [(k, C.c_int32 if k == "first" else C.c_uint64 if k == "rs_corrected" else C.c_uint32) for k in _SF_RESULT_FIELDS]


assert C.sizeof(_SfRecord) == 64 and C.sizeof(_SfResult) == 48
SF_RECORD_BYTES, SF_WORD_FAILED = 64, 0xFF
SF_FIRE_OK, SF_ZERO, SF_HEADER_VALID, SF_RS_FAILED = 1, 2, 4, 8

ETI_FRAME_BYTES = 6144
CIFS_PER_FRAME = {1: 4, 2: 1, 3: 1, 4: 2}      # ETI frames per transmission frame
FE_HISTORY_FRAMES = 15                         # ETI frames the time interleaver looks back (DABGPU_FE_HISTORY_FRAMES)

_lib = None


def load_library():
    """dlopen libdabgpu.so.  torch is imported first so that both share one
    libamdhip64 (the wheel bundles its own copy under the same soname)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DabGpuError("%s is missing: run __graft_entry__.build() (there is no CPU fallback)"
                          % LIB_PATH)
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is part of the image
        pass
    lib = C.CDLL(LIB_PATH)
    vp, sz, szp, u = C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_uint
    lib.dabgpu_create.argtypes = [C.POINTER(_Config), C.POINTER(vp)]
    lib.dabgpu_destroy.argtypes = [vp]
    lib.dabgpu_destroy.restype = None
    lib.dabgpu_last_error.argtypes = [vp]
    lib.dabgpu_last_error.restype = C.c_char_p
    lib.dabgpu_version.restype = C.c_char_p
    lib.dabgpu_get_geometry.argtypes = [vp, C.POINTER(_Geometry)]
    lib.dabgpu_set_gain.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.c_float]
    lib.dabgpu_set_fir_taps.argtypes = [vp, C.POINTER(C.c_float), sz]
    lib.dabgpu_set_fir_default_taps.argtypes = [vp]
    lib.dabgpu_set_window_overlap.argtypes = [vp, sz]
    lib.dabgpu_set_fir_boundary_mode.argtypes = [vp, C.c_int]
    lib.dabgpu_set_gain_rounding.argtypes = [vp, C.c_int]
    lib.dabgpu_debug_last_variant.argtypes = [vp, C.c_char_p, sz]
    lib.dabgpu_debug_trace.argtypes = [vp, C.c_int]
    lib.dabgpu_set_resampler.argtypes = [vp, sz, sz]
    lib.dabgpu_set_poly.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.dabgpu_set_lut.argtypes = [vp, C.c_float, C.POINTER(C.c_float)]
    for n in ("qpsk", "freq_interleave", "ofdm", "gain", "guard", "fir", "resampler", "poly"):
        getattr(lib, "dabgpu_%s_process" % n).argtypes = [vp, vp, sz, vp, sz, szp]
    lib.dabgpu_phase_reference_process.argtypes = [vp, vp, sz, szp]
    lib.dabgpu_null_symbol_process.argtypes = [vp, vp, sz, szp]
    lib.dabgpu_diff_mod_process.argtypes = [vp, vp, sz, vp, sz, vp, sz, szp]
    lib.dabgpu_signal_mux_process.argtypes = [vp, vp, sz, vp, sz, vp, sz, szp]
    lib.dabgpu_chain_out_bytes_per_frame.argtypes = [vp, u]
    lib.dabgpu_chain_out_bytes_per_frame.restype = sz
    lib.dabgpu_chain_process.argtypes = [vp, vp, sz, u, vp, sz, szp]
    lib.dabgpu_chain_process_dev.argtypes = [vp, vp, sz, u, vp, sz, szp, vp]
    lib.dabgpu_symbols_process_dev.argtypes = [vp, vp, sz, u, vp, sz, szp, vp]
    lib.dabgpu_chain_submit.argtypes = [vp, vp, sz, u]
    lib.dabgpu_chain_collect.argtypes = [vp, C.POINTER(vp), szp]
    lib.dabgpu_synchronize.argtypes = [vp]
    lib.dabgpu_set_cfr.argtypes = [vp, C.c_int, C.c_float, C.c_float]
    lib.dabgpu_get_cfr_stats.argtypes = [vp, sz, C.POINTER(_CfrStats)]
    lib.dabgpu_cic_equalizer_process.argtypes = [vp, sz, C.c_int, vp, sz, vp, sz, szp]
    lib.dabgpu_set_cic_equalizer.argtypes = [vp, C.c_int, sz, C.c_int]
    lib.dabgpu_carriers_process.argtypes = [vp, vp, sz, vp, sz, szp]
    lib.dabgpu_carriers_process_dev.argtypes = [vp, vp, sz, vp, sz, szp, vp]
    lib.dabgpu_set_tii.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.dabgpu_tii_process.argtypes = [vp, vp, sz, vp, sz, szp]
    lib.dabgpu_format_size.argtypes = [C.c_int]
    lib.dabgpu_format_size.restype = sz
    lib.dabgpu_format_process.argtypes = [vp, vp, sz, C.c_int, vp, sz, szp, szp]
    lib.dabgpu_format_process_dev.argtypes = [vp, vp, sz, C.c_int, vp, sz, szp, vp, vp]
    lib.dabgpu_set_output_format.argtypes = [vp, C.c_int]
    lib.dabgpu_get_num_clipped.argtypes = [vp, szp]
    lib.dabgpu_set_lanes.argtypes = [vp, C.c_int]
    lib.dabgpu_set_handover_frames.argtypes = [vp, C.c_int]
    lib.dabgpu_debug_lanes.argtypes = [vp, C.POINTER(C.c_int)]
    lib.dabgpu_wait_for_stream.argtypes = [vp, vp]
    lib.dabgpu_stream_wait_for.argtypes = [vp, vp]
    lib.dabgpu_post_process_dev.argtypes = [vp, vp, sz, u, vp, sz, szp, vp]
    lib.dabgpu_fir_inverse_design.argtypes = [C.POINTER(C.c_float), sz, C.POINTER(C.c_float), C.POINTER(C.c_double)]
    lib.dabgpu_stream_state_bytes.argtypes = [vp]
    lib.dabgpu_stream_state_bytes.restype = sz
    lib.dabgpu_get_stream_state.argtypes = [vp, vp, sz, szp]
    lib.dabgpu_set_stream_state.argtypes = [vp, vp, sz]
    lib.dabgpu_chain_seed.argtypes = [vp, vp, u, C.c_uint64]
    lib.dabgpu_chain_seed_dev.argtypes = [vp, vp, u, C.c_uint64, vp]
    lib.dabgpu_frontend_describe.argtypes = [vp, C.POINTER(_FeLayout)]
    lib.dabgpu_frontend_configure.argtypes = [vp, vp]
    lib.dabgpu_frontend_reset.argtypes = [vp]
    lib.dabgpu_frontend_process.argtypes = [vp, vp, sz, vp, sz, szp]
    lib.dabgpu_frontend_process_dev.argtypes = [vp, vp, sz, vp, sz, szp, vp]
    lib.dabgpu_chain_process_eti.argtypes = [vp, vp, sz, u, vp, sz, szp]
    lib.dabgpu_chain_submit_eti.argtypes = [vp, vp, sz, u]
    lib.dabgpu_frontend_state_bytes.argtypes = [vp]
    lib.dabgpu_frontend_state_bytes.restype = sz
    lib.dabgpu_frontend_get_state.argtypes = [vp, vp, sz, szp]
    lib.dabgpu_frontend_set_state.argtypes = [vp, vp, sz]
    lib.dabgpu_frontend_seed.argtypes = [vp, vp, sz, C.c_uint64]
    lib.dabgpu_frontend_seed_dev.argtypes = [vp, vp, sz, C.c_uint64, vp]
    lib.dabgpu_chain_seed_eti.argtypes = [vp, vp, sz, u, C.c_uint64]
    lib.dabgpu_chain_seed_eti_dev.argtypes = [vp, vp, sz, u, C.c_uint64, vp]
    lib.dabgpu_demod.argtypes = [vp, vp, C.c_int, sz, C.c_int, vp, vp]
    lib.dabgpu_demod_dev.argtypes = [vp, vp, C.c_int, sz, C.c_int, vp, vp, vp]
    lib.dabgpu_get_demod_stats.argtypes = [vp, sz, C.POINTER(_DemodStats)]
    lib.dabgpu_demod_check_early.argtypes = [C.c_int, C.c_int]
    lib.dabgpu_set_monitor.argtypes = [vp, C.c_int, C.c_int]
    lib.dabgpu_debug_demod_run_symbols.argtypes = [vp, C.c_int]
    lib.dabgpu_sync_dev.argtypes = [vp, vp, C.c_int, sz, C.c_int, vp]
    lib.dabgpu_sync.argtypes = [vp, vp, C.c_int, sz, C.c_int]
    lib.dabgpu_get_sync_result.argtypes = [vp, szp, C.POINTER(_SyncFrame), sz]
    lib.dabgpu_sync_extract_dev.argtypes = [vp, vp, C.c_int, sz, vp, vp]
    lib.dabgpu_sync_extract.argtypes = [vp, vp, C.c_int, sz, vp]
    lib.dabgpu_sync_check.argtypes = [C.c_int, sz, C.c_int]
    lib.dabgpu_channel_check.argtypes = [C.POINTER(_ChannelConfig)]
    lib.dabgpu_set_channel.argtypes = [vp, C.POINTER(_ChannelConfig)]
    lib.dabgpu_channel_reset.argtypes = [vp, C.c_uint64]
    lib.dabgpu_get_channel_position.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.dabgpu_channel_dev.argtypes = [vp, vp, C.c_int, sz, vp, C.c_int, vp]
    lib.dabgpu_channel.argtypes = [vp, vp, C.c_int, sz, vp, C.c_int]
    lib.dabgpu_debug_channel_run_samples.argtypes = [vp, C.c_int]
    lib.dabgpu_clock_check.argtypes = [C.c_double]
    lib.dabgpu_clock_step.argtypes = [C.c_double, C.POINTER(C.c_int64)]
    lib.dabgpu_clock_count.argtypes = [C.c_double, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.dabgpu_clock_out_max.argtypes = [sz]
    lib.dabgpu_clock_out_max.restype = sz
    lib.dabgpu_clock_phase_taps.argtypes = [C.c_int, C.POINTER(C.c_float)]
    lib.dabgpu_clock_inverse_ppm.argtypes = [C.c_double]
    lib.dabgpu_clock_inverse_ppm.restype = C.c_double
    lib.dabgpu_set_clock.argtypes = [vp, C.c_double]
    lib.dabgpu_clock_reset.argtypes = [vp, C.c_uint64]
    lib.dabgpu_get_clock_position.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.dabgpu_clock_dev.argtypes = [vp, vp, C.c_int, sz, vp, C.c_int, sz, C.POINTER(sz), vp]
    lib.dabgpu_clock.argtypes = [vp, vp, C.c_int, sz, vp, C.c_int, sz, C.POINTER(sz)]
    lib.dabgpu_debug_clock_run_samples.argtypes = [vp, C.c_int]
    tcp = C.POINTER(_TunerConfig)
    lib.dabgpu_tuner_check.argtypes = [tcp]
    lib.dabgpu_tuner_geometry.argtypes = [tcp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.dabgpu_tuner_taps.argtypes = [tcp, C.c_int, C.POINTER(C.c_float)]
    lib.dabgpu_tuner_count.argtypes = [tcp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.dabgpu_tuner_out_max.argtypes = [tcp, sz]
    lib.dabgpu_tuner_out_max.restype = sz
    lib.dabgpu_set_tuner.argtypes = [vp, tcp]
    lib.dabgpu_tuner_reset.argtypes = [vp, C.c_uint64]
    lib.dabgpu_get_tuner_position.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.dabgpu_tuner_dev.argtypes = [vp, vp, C.c_int, sz, vp, C.c_int, sz, C.POINTER(sz), vp]
    lib.dabgpu_tuner.argtypes = [vp, vp, C.c_int, sz, vp, C.c_int, sz, C.POINTER(sz)]
    lib.dabgpu_debug_tuner_run_samples.argtypes = [vp, C.c_int]
    lib.dabgpu_sco_dev.argtypes = [vp, vp, C.c_int, sz, C.c_int, vp]
    lib.dabgpu_sco.argtypes = [vp, vp, C.c_int, sz, C.c_int]
    lib.dabgpu_get_sco.argtypes = [vp, C.c_int, C.POINTER(_ScoFrame)]
    lib.dabgpu_tii_scan_dev.argtypes = [vp, vp, C.c_int, sz, C.POINTER(_TiiScanConfig), vp]
    lib.dabgpu_tii_scan.argtypes = [vp, vp, C.c_int, sz, C.POINTER(_TiiScanConfig)]
    lib.dabgpu_get_tii_scan.argtypes = [vp, C.POINTER(_TiiScanHead), C.POINTER(_TiiEntry), sz]
    lib.dabgpu_tii_scan_check.argtypes = [C.c_int, sz, C.POINTER(_TiiScanConfig)]
    lib.dabgpu_cir_dev.argtypes = [vp, vp, C.c_int, sz, C.POINTER(_CirConfig), vp]
    lib.dabgpu_cir.argtypes = [vp, vp, C.c_int, sz, C.POINTER(_CirConfig)]
    lib.dabgpu_get_cir.argtypes = [vp, C.POINTER(_CirHead), C.POINTER(_CirPath), sz]
    lib.dabgpu_get_cir_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.dabgpu_cir_check.argtypes = [C.c_int, sz, C.POINTER(_CirConfig)]
    lib.dabgpu_fic_scan_dev.argtypes = [vp, vp, sz, sz, vp]
    lib.dabgpu_fic_scan.argtypes = [vp, vp, sz, sz]
    lib.dabgpu_get_fic_result.argtypes = [vp, C.POINTER(_FicResult)]
    lib.dabgpu_get_fic_records.argtypes = [vp, vp, sz, szp]
    lib.dabgpu_get_fic_services.argtypes = [vp, vp, sz, szp, C.POINTER(_FicLabel)]
    lib.dabgpu_fic_bootstrap_frame.argtypes = [C.c_int, vp]
    lib.dabgpu_fic_make_header.argtypes = [C.POINTER(_FicResult), C.c_int, vp]
    lib.dabgpu_decode_configure_from_fic.argtypes = [vp]
    lib.dabgpu_superframe_dev.argtypes = [vp, vp, sz, sz, sz, vp, sz, szp, vp]
    lib.dabgpu_superframe.argtypes = [vp, vp, sz, sz, sz, vp, sz, szp]
    lib.dabgpu_get_superframe_result.argtypes = [vp, C.POINTER(_SfResult), vp, sz]
    lib.dabgpu_get_superframe_records.argtypes = [vp, vp, sz, szp]
    lib.dabgpu_superframe_check.argtypes = [sz, sz, sz]
    lib.dabgpu_decode_check_layout.argtypes = [C.POINTER(_FeLayout)]
    lib.dabgpu_decode_reset.argtypes = [vp]
    lib.dabgpu_decode_dev.argtypes = [vp, vp, sz, vp, sz, vp, szp, vp]
    lib.dabgpu_decode.argtypes = [vp, vp, sz, vp, sz, vp, szp]
    lib.dabgpu_get_decode_stats.argtypes = [vp, sz, C.c_int, C.POINTER(_DecodeStats)]
    lib.dabgpu_demod_soft.argtypes = [vp, vp, C.c_int, sz, C.c_int, vp, vp, vp]
    lib.dabgpu_demod_soft_dev.argtypes = [vp, vp, C.c_int, sz, C.c_int, vp, vp, vp, vp]
    lib.dabgpu_decode_soft_dev.argtypes = [vp, vp, sz, vp, sz, vp, szp, vp]
    lib.dabgpu_demod_csi.argtypes = [vp, vp, C.c_int, sz, C.c_int, vp, vp, vp]
    lib.dabgpu_demod_csi_dev.argtypes = [vp, vp, C.c_int, sz, C.c_int, vp, vp, vp, vp]
    lib.dabgpu_demod_carrier_state.argtypes = [vp, vp, C.c_int, sz, C.c_int]
    lib.dabgpu_demod_carrier_state_dev.argtypes = [vp, vp, C.c_int, sz, C.c_int, vp]
    lib.dabgpu_get_carrier_state.argtypes = [vp, sz, vp, vp, vp]
    lib.dabgpu_debug_csi_unit_weights.argtypes = [vp, C.c_int]
    lib.dabgpu_decode_soft.argtypes = [vp, vp, sz, vp, sz, vp, szp]
    lib.dabgpu_get_decode_soft_stats.argtypes = [vp, sz, C.c_int, C.POINTER(_DecodeSoftStats)]
    dp = C.POINTER(C.c_double)
    lib.dabgpu_spectrum_window.argtypes = [C.c_int, C.POINTER(C.c_float)]
    lib.dabgpu_spectrum.argtypes = [vp, vp, C.c_int, sz, C.c_int, C.c_int]
    lib.dabgpu_spectrum_dev.argtypes = [vp, vp, C.c_int, sz, C.c_int, C.c_int, vp]
    lib.dabgpu_get_spectrum.argtypes = [vp, dp, C.POINTER(_SpectrumInfo)]
    lib.dabgpu_reset_spectrum.argtypes = [vp]
    lib.dabgpu_set_spectrum_monitor.argtypes = [vp, C.c_int, C.c_int]
    lib.dabgpu_debug_spectrum_run_segments.argtypes = [vp, C.c_int]
    lib.dabgpu_debug_resampler_run_hops.argtypes = [vp, C.c_int]
    lib.dabgpu_debug_resampler_last_launch.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_uint)]
    lib.dabgpu_spectrum_check_mask.argtypes = [dp, C.c_int, C.c_double, dp, dp, C.c_int, C.c_double, C.POINTER(_MaskResult)]
    ll, fp, al = C.c_longlong, C.POINTER(C.c_float), C.POINTER(_DpdAlignment)
    lib.dabgpu_dpd_xspectrum.argtypes = [vp, vp, C.c_int, vp, sz, ll]
    lib.dabgpu_dpd_xspectrum_dev.argtypes = [vp, vp, C.c_int, vp, sz, ll, vp]
    lib.dabgpu_get_dpd_xspectrum.argtypes = [vp, dp, dp, dp, C.POINTER(C.c_uint64)]
    lib.dabgpu_dpd_solve_alignment.argtypes = [dp, dp, dp, al]
    lib.dabgpu_dpd_align.argtypes = [vp, vp, C.c_int, vp, sz, al]
    lib.dabgpu_dpd_align_dev.argtypes = [vp, vp, C.c_int, vp, sz, al, vp]
    lib.dabgpu_dpd_delay_taps.argtypes = [C.c_double, fp]
    lib.dabgpu_dpd_measure.argtypes = [vp, vp, C.c_int, vp, sz, al, C.c_float, C.c_int, C.c_int]
    lib.dabgpu_dpd_measure_dev.argtypes = [vp, vp, C.c_int, vp, sz, al, C.c_float, C.c_int, C.c_int, vp]
    lib.dabgpu_get_dpd_stats.argtypes = [vp, C.POINTER(_DpdStats)]
    lib.dabgpu_reset_dpd.argtypes = [vp]
    lib.dabgpu_debug_dpd_run_segments.argtypes = [vp, C.c_int]
    lib.dabgpu_debug_dpd_tile.argtypes = [vp, C.c_int]
    lib.dabgpu_dpd_fit_poly.argtypes = [C.POINTER(_DpdStats), C.c_int, C.c_uint64, C.c_int, C.c_double, fp, fp, C.c_double,
                                        C.c_double, fp, fp, C.POINTER(_DpdFitInfo)]
    _lib = lib
    return lib


def demod_check_early(mode, early):
    """Host only (needs the library, no device): raises DabGpuError when `early` lies outside the cyclic prefix of the mode's
    data symbols, with the message demod() / set_monitor() give."""
    lib = load_library()
    if lib.dabgpu_demod_check_early(int(mode), int(early)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())


def sync_check(mode, n_samples, max_shift=31):
    """Host only (needs the library, no device): raises DabGpuError when sync() would refuse a capture of n_samples in this mode
    or this max_shift, with the message it gives."""
    lib = load_library()
    if int(n_samples) < 0:
        raise DabGpuError("sync: n_samples must not be negative")
    if lib.dabgpu_sync_check(int(mode), int(n_samples), int(max_shift)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())


def _tii_scan_config(early, old_variant, min_ratio, min_rel):
    cfg = _TiiScanConfig()
    cfg.early, cfg.old_variant, cfg.min_ratio, cfg.min_rel = int(early), int(bool(old_variant)), float(min_ratio), float(min_rel)
    return cfg


def tii_scan_check(mode, n_frames, early, old_variant=False, min_ratio=12.0, min_rel=1e-3):
    """Host only (needs the library, no device): raises DabGpuError when tii_scan() would refuse these settings in this mode,
    with the message it gives (n_frames against max_frames is the context's to check)."""
    lib = load_library()
    if int(n_frames) < 0:
        raise DabGpuError("tii_scan: n_frames must lie in 2 ... max_frames")
    cfg = _tii_scan_config(early, old_variant, min_ratio, min_rel)
    if lib.dabgpu_tii_scan_check(int(mode), int(n_frames), C.byref(cfg)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())


def _cir_config(early, window, min_ratio, min_rel):
    cfg = _CirConfig()
    cfg.early, cfg.window, cfg.min_ratio, cfg.min_rel = int(early), int(window), float(min_ratio), float(min_rel)
    return cfg


def cir_check(mode, n_frames, early, window=1, min_ratio=20.0, min_rel=1e-3):
    """Host only (needs the library, no device): raises DabGpuError when cir() would refuse these settings in this mode, with
    the message it gives (n_frames against max_frames is the context's to check)."""
    lib = load_library()
    if int(n_frames) < 0:
        raise DabGpuError("cir: n_frames must lie in 1 ... max_frames")
    cfg = _cir_config(early, window, min_ratio, min_rel)
    if lib.dabgpu_cir_check(int(mode), int(n_frames), C.byref(cfg)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())


def _channel_config(paths, sigma, seed, rate_hz):
    """The C structure of a channel configuration; what cannot be written into it is refused here, with the library's words."""
    paths = list(paths)
    if len(paths) > CH_MAX_PATHS:
        raise DabGpuError("channel: at most 64 paths (DABGPU_CH_MAX_PATHS)")
    cfg = _ChannelConfig()
    cfg.n_paths, cfg.sigma, cfg.seed, cfg.rate_hz = len(paths), float(sigma), int(seed) & (2 ** 64 - 1), float(rate_hz)
    for i, (delay, gain, doppler_hz) in enumerate(paths):
        if not 0 <= int(delay) <= CH_MAX_DELAY:
            raise DabGpuError("channel: a path's delay is 0 ... 2047 samples (DABGPU_CH_MAX_DELAY)")
        g = np.complex64(gain)
        cfg.paths[i].delay, cfg.paths[i].gain_re, cfg.paths[i].gain_im = int(delay), float(g.real), float(g.imag)
        cfg.paths[i].doppler_hz = float(doppler_hz)
    return cfg


def channel_check(paths, sigma=0.0, seed=0, rate_hz=2048000.0):
    """Host only (needs the library, no device): raises DabGpuError when set_channel() would refuse these settings, with the
    message it gives.  paths: (delay, gain, doppler_hz) tuples, the gain complex."""
    lib = load_library()
    cfg = _channel_config(paths, sigma, seed, rate_hz)
    if lib.dabgpu_channel_check(C.byref(cfg)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())


def clock_check(ppm):
    """Host only (needs the library, no device): raises DabGpuError when set_clock() would refuse this offset, with the
    message it gives."""
    lib = load_library()
    if lib.dabgpu_clock_check(float(ppm)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())


def clock_step(ppm):
    """Host only: the clock's step, llrint(ppm 1e-6 2^64), as a Python integer."""
    lib = load_library()
    step = C.c_int64()
    if lib.dabgpu_clock_step(float(ppm), C.byref(step)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())
    return int(step.value)


def clock_count(ppm, T):
    """Host only: M(T), the outputs the clock has written once T input samples have arrived."""
    lib = load_library()
    if not 0 <= int(T) < 2 ** 64:
        raise DabGpuError("clock: the stream's position must not exceed 2^62")
    m = C.c_uint64()
    if lib.dabgpu_clock_count(float(ppm), int(T), C.byref(m)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())
    return int(m.value)


def clock_out_max(n_in):
    """Host only: an upper bound of the outputs of any clock call that brings n_in samples."""
    return int(load_library().dabgpu_clock_out_max(int(n_in)))


def clock_phase_taps(p):
    """Host only: row p (0 ... 512) of the clock's tap table, 32 fp32 taps."""
    lib = load_library()
    out = np.empty(32, np.float32)
    if lib.dabgpu_clock_phase_taps(int(p), out.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())
    return out


def clock_inverse_ppm(ppm):
    """Host only: the setting that undoes an offset of ppm, -ppm / (1 + ppm 1e-6)."""
    return float(load_library().dabgpu_clock_inverse_ppm(float(ppm)))


def _tuner_config(in_rate, selectivity, offset_hz):
    """The C structure of a tuner setting; what cannot be written into it is refused here, with the library's words."""
    if not 0 <= int(in_rate) < 2 ** 32:
        raise DabGpuError("tuner: in_rate_hz must not be below 2048000" if int(in_rate) < 0
                          else "tuner: in_rate_hz must not exceed 8 x 2048000 (M <= 8 L)")
    if not -2 ** 31 <= int(selectivity) < 2 ** 31:
        raise DabGpuError("tuner: selectivity is 0 (wide) or 1 (channel)")
    return _TunerConfig(int(in_rate), int(selectivity), float(offset_hz))


def tuner_check(in_rate, selectivity=0, offset_hz=0.0):
    """Host only (needs the library, no device): raises DabGpuError when set_tuner() would refuse this setting, with the
    message it gives."""
    lib = load_library()
    cfg = _tuner_config(in_rate, selectivity, offset_hz)
    if lib.dabgpu_tuner_check(C.byref(cfg)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())


def tuner_geometry(in_rate, selectivity=0, offset_hz=0.0):
    """Host only: (L, M, P) of a tuner setting: the ratio 2048000 / in_rate = L / M in lowest terms and the taps per output."""
    lib = load_library()
    cfg = _tuner_config(in_rate, selectivity, offset_hz)
    L, M, P = C.c_int(), C.c_int(), C.c_int()
    if lib.dabgpu_tuner_geometry(C.byref(cfg), C.byref(L), C.byref(M), C.byref(P)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())
    return int(L.value), int(M.value), int(P.value)


def tuner_taps(in_rate, selectivity, p):
    """Host only: row p (0 ... L - 1) of the tuner's tap table, P fp32 taps."""
    lib = load_library()
    cfg = _tuner_config(in_rate, selectivity, 0.0)
    out = np.empty(tuner_geometry(in_rate, selectivity)[2], np.float32)
    if lib.dabgpu_tuner_taps(C.byref(cfg), int(p), out.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())
    return out


def tuner_count(in_rate, selectivity, T):
    """Host only: M(T), the outputs the tuner has written once T input samples have arrived."""
    lib = load_library()
    if not 0 <= int(T) < 2 ** 64:
        raise DabGpuError("tuner: the stream's position must not exceed 2^50")
    cfg = _tuner_config(in_rate, selectivity, 0.0)
    m = C.c_uint64()
    if lib.dabgpu_tuner_count(C.byref(cfg), int(T), C.byref(m)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())
    return int(m.value)


def tuner_out_max(in_rate, selectivity, n_in):
    """Host only: an upper bound of the outputs of any tuner call that brings n_in samples."""
    tuner_check(in_rate, selectivity)
    cfg = _tuner_config(in_rate, selectivity, 0.0)
    return int(load_library().dabgpu_tuner_out_max(C.byref(cfg), int(n_in)))


def channel_sigma(power, cn_db):
    """The channel's sigma (per component) that puts a signal of mean power `power` at C/N cn_db: sqrt(power / 10^(cn_db / 10) / 2)."""
    return float(np.sqrt(float(power) / 10.0 ** (float(cn_db) / 10.0) / 2.0))


def rayleigh_paths(delays, powers_db, doppler_hz, n_sinusoids, seed):
    """Host only: a sum-of-sinusoids fading profile as a path list for set_channel().  Per delay, n_sinusoids paths of equal
    power (together 10^(powers_db / 10)), Doppler doppler_hz cos(alpha_k) with alpha_k = 2 pi (k + u) / n_sinusoids, u and the
    phases drawn from numpy's RandomState(seed).  A convenience: no statistical claim is made for it."""
    delays, powers_db = [int(d) for d in delays], [float(p) for p in powers_db]
    n_sinusoids = int(n_sinusoids)
    if len(delays) != len(powers_db) or n_sinusoids < 1:
        raise DabGpuError("rayleigh_paths: one power per delay, at least one sinusoid")
    if len(delays) * n_sinusoids > CH_MAX_PATHS:
        raise DabGpuError("channel: at most 64 paths (DABGPU_CH_MAX_PATHS)")
    rs = np.random.RandomState(int(seed))
    paths = []
    for d, p_db in zip(delays, powers_db):
        amp = np.sqrt(10.0 ** (p_db / 10.0) / n_sinusoids)
        alpha = 2.0 * np.pi * (np.arange(n_sinusoids) + rs.uniform()) / n_sinusoids
        phase = rs.uniform(0.0, 2.0 * np.pi, n_sinusoids)
        for k in range(n_sinusoids):
            paths.append((d, complex(amp * np.exp(1j * phase[k])), float(doppler_hz) * float(np.cos(alpha[k]))))
    return paths


def decode_check_layout(frame):
    """Host only (needs the library, no device): raises DabGpuError when the layout of this ETI frame is one the front-end
    refuses, or one the channel decoder refuses (two sub-channels on one capacity unit)."""
    lib = load_library()
    frame = np.ascontiguousarray(frame, np.uint8).reshape(-1)
    if frame.size != ETI_FRAME_BYTES:
        raise DabGpuError("frontend: ETI frames are 6144 bytes")
    lay = _FeLayout()
    if lib.dabgpu_frontend_describe(frame.ctypes.data, C.byref(lay)) != 0 or lib.dabgpu_decode_check_layout(C.byref(lay)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())


def fic_bootstrap_frame(mode):
    """Host only (needs the library, no device): the 6144-byte ETI frame of an ensemble with FICF = 1 and NST = 0 in `mode`.
    frontend_configure() on it leaves a decoder that decodes the FIC alone -- where a blind receiver starts."""
    lib = load_library()
    frame = np.empty(ETI_FRAME_BYTES, np.uint8)
    if lib.dabgpu_fic_bootstrap_frame(int(mode), frame.ctypes.data) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())
    return frame


def _fic_label_dict(l):
    return None if not l.kind else dict(kind=int(l.kind), charset=int(l.charset), id=int(l.id), flag=int(l.flag),
                                        text=bytes(bytearray(l.text)))


def _fic_result_dict(r):
    d = {k: int(getattr(r, k)) for k in _FIC_RESULT_FIELDS if k != "reserved"}
    d["figs_type"], d["fig0_ext"] = list(r.figs_type), list(r.fig0_ext)
    d["sub"] = [{k: int(getattr(r.sub[i], k)) for k in _FIC_SUBCH_FIELDS} for i in range(min(r.n_subch, 64))]
    return d


def _fic_result_struct(result):
    """a result dictionary of fic_result() (or a _FicResult) as the C structure"""
    if isinstance(result, _FicResult):
        return result
    r = _FicResult()
    for k in _FIC_RESULT_FIELDS:
        setattr(r, k, int(result.get(k, 0)))
    for name in ("figs_type", "fig0_ext"):
        for i, v in enumerate(result.get(name, ())):
            getattr(r, name)[i] = int(v)
    for i, sub in enumerate(result.get("sub", ())[:64]):
        for k in _FIC_SUBCH_FIELDS:
            setattr(r.sub[i], k, int(sub.get(k, 0)))
    return r


def fic_make_header(result, mode):
    """Host only (needs the library, no device): the ETI frame frontend_configure() wants, from a result of fic_result() -- FC and
    one STC word per sub-channel in ascending SubChId.  Raises DabGpuError when the result does not say how the ensemble is laid
    out (no FIG 0/1, a redefinition inside the capture, a form that is not supported) or says a layout the front-end or the
    decoder refuses."""
    lib = load_library()
    r = _fic_result_struct(result)
    frame = np.empty(ETI_FRAME_BYTES, np.uint8)
    if lib.dabgpu_fic_make_header(C.byref(r), int(mode), frame.ctypes.data) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())
    return frame


def superframe_check(n_images, offset, framesize):
    """Host only (needs the library, no device): raises DabGpuError with the refusal superframe() would give this shape."""
    lib = load_library()
    if lib.dabgpu_superframe_check(int(n_images), int(offset), int(framesize)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())


def superframe_record_dict(row):
    """one row of superframe_records() as a dict of the fields of dabgpu_sf_record"""
    r = _SfRecord.from_buffer_copy(bytes(row))
    d = {k: int(getattr(r, k)) for k, t in _SfRecord._fields_ if not k.startswith("reserved") and k not in ("au_start", "cw_errors")}
    d["au_start"] = [int(v) for v in r.au_start]
    d["cw_errors"] = [int(v) for v in r.cw_errors]
    return d


def superframe_aus(out, result, records):
    """The access units of a call's accepted superframes, sliced on the host: (aus, crc_ok) -- aus: the AUs without their CRC as
    bytes, in stream order; crc_ok: one bool each.  out, result, records: what superframe() / superframe_result() /
    superframe_records() gave for the call."""
    out = np.frombuffer(out, np.uint8) if isinstance(out, (bytes, bytearray)) else np.ascontiguousarray(out, np.uint8)
    out = out.reshape(result["candidates"], -1)
    aus, ok = [], []
    for f in result["accepted"]:
        r = superframe_record_dict(records[f])
        for k in range(r["num_aus"]):
            aus.append(out[f, r["au_start"][k]:r["au_start"][k + 1] - 2].tobytes())
            ok.append(bool(r["au_ok"] >> k & 1))
    return aus, ok


def decode_reference(eti, e, n):
    """The reference rows of a decode() call: the call that brings ETI frames e ... e + n - 1 of the stream `eti`
    ((frames, 6144) uint8) returns frames e - 15 ... e + n - 16, so row i is frame e + i - 15 -- zero where that lies before
    the start of the stream (the lead-in outputs, which are not compared)."""
    eti = np.ascontiguousarray(eti, np.uint8).reshape(-1, ETI_FRAME_BYTES)
    ref = np.zeros((n, ETI_FRAME_BYTES), np.uint8)
    for i in range(n):
        k = e + i - FE_HISTORY_FRAMES
        if 0 <= k < eti.shape[0]:
            ref[i] = eti[k]
    return ref


def spectrum_window(window):
    """Host only (needs the library, no device): the 2048-entry fp32 window table the spectrum kernel multiplies by --
    0 rectangular, 1 Hann, 2 four-term Blackman-Harris, periodic form."""
    lib = load_library()
    out = np.empty(SPECTRUM_NFFT, np.float32)
    if lib.dabgpu_spectrum_window(int(window), out.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())
    return out


def spectrum_freqs(rate_hz, nfft=SPECTRUM_NFFT):
    """The frequency of every bin in FFT order: f_k = (k < nfft/2 ? k : k - nfft) rate_hz / nfft."""
    k = np.arange(nfft)
    return np.where(k < nfft // 2, k, k - nfft) * (float(rate_hz) / nfft)


def check_mask(raw, rate_hz, mask=(), oob_from_hz=OOB_FROM_HZ):
    """Host only: dabgpu_spectrum_check_mask on raw sums in FFT order.  mask: (offset_hz, limit_db) pairs, offsets strictly
    increasing (empty: only ref and the out-of-band maximum are formed).  Returns a dict of the result's fields."""
    lib = load_library()
    raw = np.ascontiguousarray(raw, np.float64).reshape(-1)
    pts = np.ascontiguousarray(mask, np.float64).reshape(-1, 2)
    offs, lim = np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1])
    dp = C.POINTER(C.c_double)
    res = _MaskResult()
    if lib.dabgpu_spectrum_check_mask(raw.ctypes.data_as(dp), raw.size, float(rate_hz), offs.ctypes.data_as(dp),
                                      lim.ctypes.data_as(dp), offs.size, float(oob_from_hz), C.byref(res)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())
    return {k: getattr(res, k) for k, _ in _MaskResult._fields_}


def _alignment_dict(a):
    return {"lag": int(a.lag), "tau": float(a.tau), "gain": complex(a.gain_re, a.gain_im), "coherence": float(a.coherence)}


def _alignment_struct(al):
    """None, or a dict with lag / tau / gain (as dpd_align returns it) -> (_DpdAlignment or None)"""
    if al is None:
        return None
    g = complex(al.get("gain", 1.0))
    return _DpdAlignment(int(al.get("lag", 0)), float(al.get("tau", 0.0)), g.real, g.imag, float(al.get("coherence", 0.0)))


def dpd_solve_alignment(S, p_tx, p_rx):
    """Host only: dabgpu_dpd_solve_alignment on a cross-spectrum (S: 2048 complex, p_tx / p_rx: 2048 real, FFT order).
    Returns a dict: lag, tau, gain (complex), coherence; rx[i + lag + tau] belongs to tx[i]."""
    lib = load_library()
    s2 = np.ascontiguousarray(S, np.complex128).reshape(-1)
    pt = np.ascontiguousarray(p_tx, np.float64).reshape(-1)
    pr = np.ascontiguousarray(p_rx, np.float64).reshape(-1)
    if s2.size != SPECTRUM_NFFT or pt.size != SPECTRUM_NFFT or pr.size != SPECTRUM_NFFT:
        raise DabGpuError("dpd_solve_alignment: S, p_tx and p_rx hold 2048 bins each")
    dp = C.POINTER(C.c_double)
    a = _DpdAlignment()
    if lib.dabgpu_dpd_solve_alignment(s2.view(np.float64).ctypes.data_as(dp), pt.ctypes.data_as(dp), pr.ctypes.data_as(dp),
                                      C.byref(a)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())
    return _alignment_dict(a)


def dpd_delay_taps(tau):
    """Host only: the 32 fp32 taps of the fractional-delay filter the statistics kernel runs on rx (Kaiser-windowed sinc,
    beta = 10, centred on tap 15; tau = 0 is the unit impulse)."""
    lib = load_library()
    out = np.empty(DPD_TAPS, np.float32)
    if lib.dabgpu_dpd_delay_taps(float(tau), out.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())
    return out


def _stats_struct(stats):
    st = _DpdStats()
    n = int(stats["n_bins"])
    if not 1 <= n <= DPD_MAX_BINS:
        raise DabGpuError("dpd: n_bins is 1 ... 256")
    st.n_bins, st.peak = n, float(stats["peak"])
    for name in ("count", "sum_tx", "sum_rx", "sum_phase"):
        v = np.asarray(stats[name]).reshape(-1)
        if v.size < n:
            raise DabGpuError("dpd: %s holds fewer than n_bins entries" % name)
        arr = getattr(st, name)
        for b in range(n):
            arr[b] = int(v[b]) if name == "count" else float(v[b])
    return st


def dpd_fit_poly(stats, basis="magsq", min_count=1, weighted=True, tx_min=0.0, prev_am=None, prev_pm=None, lr_am=1.0,
                 lr_pm=1.0):
    """Host only: dabgpu_dpd_fit_poly on per-bin statistics (the dict Modulator.dpd_stats() returns, or any dict with
    n_bins, peak, count, sum_tx, sum_rx, sum_phase).  basis "magsq" (the default) gives the coefficients set_poly takes;
    "reference" restates the reference's Model_Poly.  Returns (am, pm, info)."""
    lib = load_library()
    st = _stats_struct(stats)
    fp = C.POINTER(C.c_float)
    am, pm = np.zeros(5, np.float32), np.zeros(5, np.float32)
    pa = None if prev_am is None else np.ascontiguousarray(prev_am, np.float32).reshape(5)
    pp = None if prev_pm is None else np.ascontiguousarray(prev_pm, np.float32).reshape(5)
    info = _DpdFitInfo()
    if lib.dabgpu_dpd_fit_poly(C.byref(st), DPD_BASIS[basis] if isinstance(basis, str) else int(basis), int(min_count),
                               int(bool(weighted)), float(tx_min), None if pa is None else pa.ctypes.data_as(fp),
                               None if pp is None else pp.ctypes.data_as(fp), float(lr_am), float(lr_pm),
                               am.ctypes.data_as(fp), pm.ctypes.data_as(fp), C.byref(info)) != 0:
        raise DabGpuError(lib.dabgpu_last_error(None).decode())
    return am, pm, {k: getattr(info, k) for k, _ in _DpdFitInfo._fields_}


def fir_inverse_design(taps):
    """Host-side helper (no device): the 160-tap inverse of a FIR of up to 45 taps on the occupied carriers of a Mode I symbol,
    as the frame kernel's equalised-boundary variant uses it.  Returns (ok, g, fit)."""
    lib = load_library()
    taps = np.ascontiguousarray(taps, np.float32)
    g = np.zeros(160, np.float32)
    fit = C.c_double()
    rc = lib.dabgpu_fir_inverse_design(_f32p(taps), taps.size, _f32p(g), C.byref(fit))
    return rc == 0, g, fit.value


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Modulator:
    """One device context: geometry tables, settings and scratch for one stream.

    Method names follow the reference plugins (src/DabModulator.cpp:385-419);
    errors the reference throws as std::runtime_error surface as DabGpuError
    with the same message.
    """

    def __init__(self, mode=1, device=0, max_frames=1, chunks_per_frame=0):
        self._lib = load_library()
        cfg = _Config(mode, device, max_frames, chunks_per_frame)
        h = C.c_void_p()
        rc = self._lib.dabgpu_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise DabGpuError("dabgpu_create: " + self._lib.dabgpu_last_error(None).decode())
        self._h = h
        g = _Geometry()
        self._lib.dabgpu_get_geometry(self._h, C.byref(g))
        self.geometry = {n: getattr(g, n) for n, _ in _Geometry._fields_}
        self.device = device
        self.max_frames = int(max_frames)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dabgpu_destroy(self._h)
            self._h = None

    __del__ = close

    def _chk(self, rc):
        if rc != 0:
            raise DabGpuError(self._lib.dabgpu_last_error(self._h).decode())

    # ---- settings ----------------------------------------------------------
    def set_gain(self, mode=GAIN_VAR, digital=1.0, normalise=1.0, var_variance=4.0):
        self._chk(self._lib.dabgpu_set_gain(self._h, mode, digital, normalise, var_variance))

    def set_fir_taps(self, taps=None):
        if taps is None:
            self._chk(self._lib.dabgpu_set_fir_default_taps(self._h))
        else:
            t = np.ascontiguousarray(taps, np.float32)
            self._chk(self._lib.dabgpu_set_fir_taps(self._h, _f32p(t), t.size))

    def set_window_overlap(self, overlap):
        self._chk(self._lib.dabgpu_set_window_overlap(self._h, overlap))

    def set_resampler(self, in_rate, out_rate):
        self._chk(self._lib.dabgpu_set_resampler(self._h, in_rate, out_rate))

    def set_poly(self, am, pm):
        a = np.ascontiguousarray(am, np.float32)
        p = np.ascontiguousarray(pm, np.float32)
        assert a.size == 5 and p.size == 5
        self._chk(self._lib.dabgpu_set_poly(self._h, _f32p(a), _f32p(p)))

    def set_lut(self, scalefactor, lut):
        t = np.ascontiguousarray(lut, np.float32)
        assert t.size == 32
        self._chk(self._lib.dabgpu_set_lut(self._h, float(scalefactor), _f32p(t)))

    # ---- per-stage, host arrays -------------------------------------------
    def _stage(self, name, x, out_bytes, dtype=np.complex64):
        x = np.ascontiguousarray(x)
        out = np.empty(max(out_bytes, 1), np.uint8)
        n = C.c_size_t()
        fn = getattr(self._lib, "dabgpu_%s_process" % name)
        self._chk(fn(self._h, x.ctypes.data, x.nbytes, out.ctypes.data, out_bytes, C.byref(n)))
        return out[:n.value].view(dtype)

    def qpsk(self, bits):
        bits = np.ascontiguousarray(bits, np.uint8)
        return self._stage("qpsk", bits, bits.size * 32)

    def freq_interleave(self, x):
        x = np.ascontiguousarray(x, np.complex64)
        return self._stage("freq_interleave", x, x.nbytes)

    def phase_reference(self):
        nbytes = self.geometry["carriers"] * 8
        out = np.empty(nbytes, np.uint8)
        n = C.c_size_t()
        self._chk(self._lib.dabgpu_phase_reference_process(self._h, out.ctypes.data, nbytes, C.byref(n)))
        return out[:n.value].view(np.complex64)

    def null_symbol(self):
        nbytes = self.geometry["carriers"] * 8
        out = np.empty(nbytes, np.uint8)
        n = C.c_size_t()
        self._chk(self._lib.dabgpu_null_symbol_process(self._h, out.ctypes.data, nbytes, C.byref(n)))
        return out[:n.value].view(np.complex64)

    def diff_mod(self, phase, data):
        phase = np.ascontiguousarray(phase, np.complex64)
        data = np.ascontiguousarray(data, np.complex64)
        nbytes = phase.nbytes + data.nbytes
        out = np.empty(max(nbytes, 1), np.uint8)
        n = C.c_size_t()
        self._chk(self._lib.dabgpu_diff_mod_process(self._h, phase.ctypes.data, phase.nbytes,
                                                    data.ctypes.data, data.nbytes,
                                                    out.ctypes.data, nbytes, C.byref(n)))
        return out[:n.value].view(np.complex64)

    def signal_mux(self, first, rest):
        first = np.ascontiguousarray(first, np.complex64)
        rest = np.ascontiguousarray(rest, np.complex64)
        nbytes = first.nbytes + rest.nbytes
        out = np.empty(max(nbytes, 1), np.uint8)
        n = C.c_size_t()
        self._chk(self._lib.dabgpu_signal_mux_process(self._h, first.ctypes.data, first.nbytes,
                                                      rest.ctypes.data, rest.nbytes,
                                                      out.ctypes.data, nbytes, C.byref(n)))
        return out[:n.value].view(np.complex64)

    def ofdm(self, x):
        x = np.ascontiguousarray(x, np.complex64)
        g = self.geometry
        return self._stage("ofdm", x, (g["nb_symbols"] + 1) * g["spacing"] * 8)

    def gain(self, x):
        x = np.ascontiguousarray(x, np.complex64)
        return self._stage("gain", x, x.nbytes)

    def guard(self, x):
        x = np.ascontiguousarray(x, np.complex64)
        return self._stage("guard", x, self.geometry["tf_samples"] * 8)

    def fir(self, x):
        x = np.ascontiguousarray(x, np.complex64)
        return self._stage("fir", x, x.nbytes)

    def resample(self, x, ratio_hint=8):
        x = np.ascontiguousarray(x, np.complex64)
        return self._stage("resampler", x, x.nbytes * ratio_hint)

    def poly(self, x):
        x = np.ascontiguousarray(x, np.complex64)
        return self._stage("poly", x, x.nbytes)

    def set_cfr(self, enable, clip=1.0, error_clip=1.0):
        """OfdmGenerator RC parameters cfr / clip / errorclip (src/OfdmGenerator.cpp:376-404)."""
        self._chk(self._lib.dabgpu_set_cfr(self._h, int(enable), clip, error_clip))

    def cfr_stats(self, frame=0):
        """Raw CFR statistics of frame `frame` of the most recent call with CFR on."""
        st = _CfrStats()
        self._chk(self._lib.dabgpu_get_cfr_stats(self._h, frame, C.byref(st)))
        n = st.nb_symbols
        d = {k: getattr(st, k) for k in ("num_clip", "num_error_clip", "num_samples", "mer_symbol",
                                         "mer_sum_iq", "mer_sum_delta", "nb_symbols")}
        d["papr_before"] = np.array([[st.papr_before[i][0], st.papr_before[i][1]] for i in range(n)])
        d["papr_after"] = np.array([[st.papr_after[i][0], st.papr_after[i][1]] for i in range(n)])
        return d

    def cic_equalizer(self, x, spacing, R):
        """CicEqualizer(carriers, spacing, R)::process."""
        x = np.ascontiguousarray(x, np.complex64)
        out = np.empty_like(x)
        n = C.c_size_t()
        self._chk(self._lib.dabgpu_cic_equalizer_process(self._h, spacing, R, x.ctypes.data, x.nbytes,
                                                         out.ctypes.data, out.nbytes, C.byref(n)))
        return out

    def set_cic_equalizer(self, enable, spacing=0, R=0):
        """CicEqualizer(carriers, spacing, R) between cifSig and cifOfdm of every chain call (src/DabModulator.cpp:155-176,
        :399): the chain then forms the equalised carriers first (one kernel) and runs from carriers.  Off by default."""
        self._chk(self._lib.dabgpu_set_cic_equalizer(self._h, int(bool(enable)), int(spacing), int(R)))

    def carriers(self, bits):
        """Host path: coded bits (n_frames x tf_input_bytes uint8) -> the SignalMultiplexer output, complex64
        (n_frames x (nb_symbols + 1) * carriers), with the TII and CIC settings applied; advances the TII frame parity."""
        bits = np.ascontiguousarray(bits, np.uint8).reshape(-1)
        g = self.geometry
        per_out = (g["nb_symbols"] + 1) * g["carriers"]
        n = bits.size // g["tf_input_bytes"]
        out = np.empty(max(n, 1) * per_out, np.complex64)
        ob = C.c_size_t()
        self._chk(self._lib.dabgpu_carriers_process(self._h, bits.ctypes.data, bits.size, out.ctypes.data, out.nbytes,
                                                    C.byref(ob)))
        return out[:ob.value // 8].reshape(n, per_out)

    def carriers_dev(self, d_bits, n_frames, d_out, stream=None):
        """Device path on torch tensors (coded bits -> carriers), asynchronous on the stream as chain_dev."""
        s = self._stream_handle(d_bits, stream)
        ob = C.c_size_t()
        self._chk(self._lib.dabgpu_carriers_process_dev(self._h, d_bits.data_ptr(), n_frames, d_out.data_ptr(),
                                                        d_out.numel() * d_out.element_size(), C.byref(ob), s))
        if not s:
            self.synchronize()
        return ob.value

    def set_tii(self, enable, comb=0, pattern=0, old_variant=False):
        self._chk(self._lib.dabgpu_set_tii(self._h, int(enable), comb, pattern, int(old_variant)))

    def tii(self, phase):
        """TII::process: phase reference symbol -> TII symbol (or zeros on idle calls)."""
        x = np.ascontiguousarray(phase, np.complex64)
        return self._stage("tii", x, x.nbytes)

    def format_convert(self, x, fmt):
        """FormatConverter (float input): returns (integer array, clipped components).
        An unknown format raises like the reference (src/FormatConverter.cpp:171-173)."""
        x = np.ascontiguousarray(x).view(np.float32).ravel()
        code, dt = FORMATS.get(fmt, (0, np.uint8))
        out = np.empty(x.size, dt)
        ob, nc = C.c_size_t(), C.c_size_t()
        self._chk(self._lib.dabgpu_format_process(self._h, x.ctypes.data, x.nbytes, code, out.ctypes.data,
                                                  out.nbytes, C.byref(ob), C.byref(nc)))
        return out[:ob.value // out.itemsize], int(nc.value)

    def format_convert_dev(self, d_in, fmt, d_out, d_clipped=None, stream=None):
        """Device path: d_in complex64/float32 tensor -> d_out integer tensor (asynchronous);
        d_clipped (int64 tensor of one element, optional) is incremented."""
        code = FORMATS.get(fmt, (0, None))[0]
        n = d_in.numel() * (2 if d_in.is_complex() else 1)
        ob = C.c_size_t()
        s = self._stream_handle(d_in, stream)
        self._chk(self._lib.dabgpu_format_process_dev(
            self._h, d_in.data_ptr(), n, code, d_out.data_ptr(), d_out.numel() * d_out.element_size(),
            C.byref(ob), d_clipped.data_ptr() if d_clipped is not None else None, s))
        if not s:
            self.synchronize()
        return ob.value

    # ---- fused chain -------------------------------------------------------
    def set_fir_boundary_mode(self, direct):
        """False (default): boundary outputs of the fused FIRFilter through the taps' inverse where one exists;
        True: always the direct sum over the unfiltered samples (packed dual transform)."""
        self._chk(self._lib.dabgpu_set_fir_boundary_mode(self._h, 1 if direct else 0))

    def set_gain_rounding(self, reference):
        """False (default): gain mode var from the exact variance inside the frame kernel; True: chain calls replay the
        reference's running fp32 recurrence (src/GainControl.cpp:251-340) -- its scalars bit for bit, separate kernels."""
        self._chk(self._lib.dabgpu_set_gain_rounding(self._h, 1 if reference else 0))

    def trace(self, enable=True):
        """Turn the launch trace behind last_variant() on or off (off by default)."""
        self._chk(self._lib.dabgpu_debug_trace(self._h, 1 if enable else 0))

    def last_variant(self):
        """The kernels the most recent chain call launched (dabgpu_debug_last_variant), as a list of names."""
        buf = C.create_string_buffer(4096)
        self._chk(self._lib.dabgpu_debug_last_variant(self._h, buf, len(buf)))
        return [k for k in buf.value.decode().split("; ") if k]

    def set_output_format(self, fmt=None):
        """FormatConverter as the chain's last step: None / "complexf", or "s16" / "u8" / "s8"."""
        code = 0 if fmt in (None, "complexf") else FORMATS.get(fmt, (99, None))[0]
        self._chk(self._lib.dabgpu_set_output_format(self._h, code))
        self._out_dtype = np.complex64 if code == 0 else FORMATS[fmt][1]

    def num_clipped(self):
        """Clipped components of the most recent chain call (FormatConverter::get_num_clipped_samples)."""
        n = C.c_size_t()
        self._chk(self._lib.dabgpu_get_num_clipped(self._h, C.byref(n)))
        return int(n.value)

    def out_bytes_per_frame(self, stages):
        return self._lib.dabgpu_chain_out_bytes_per_frame(self._h, stages)

    def out_samples_per_frame(self, stages):
        """Complex samples per frame (8 bytes each as complexf; 4 / 2 with an integer output format)."""
        dt = np.dtype(getattr(self, "_out_dtype", np.complex64))
        per_sample = 8 if dt == np.complex64 else 2 * dt.itemsize
        return self._lib.dabgpu_chain_out_bytes_per_frame(self._h, stages) // per_sample

    def chain(self, bits, stages, out=None):
        """Host path: bits (n_frames x tf_input_bytes uint8) -> complex64 (n_frames x samples), or the integer
        components (n_frames x 2 * samples) when an output format is set.  `out`: a buffer to reuse (what a ModPlugin's
        Buffer is: allocated once, Buffer::setLength only grows) -- a fresh 100 MB numpy array per call is 25 000 page
        faults inside the copy."""
        bits = np.ascontiguousarray(bits, np.uint8).reshape(-1)
        per = self.geometry["tf_input_bytes"]
        if bits.size % per:
            raise DabGpuError("chain: input size not valid")
        n = bits.size // per
        dt = np.dtype(getattr(self, "_out_dtype", np.complex64))
        per_out = self.out_bytes_per_frame(stages) // dt.itemsize
        if out is None:
            out = np.empty(n * per_out, dt)
        # (checked BEFORE any reshape: reshaping a non-contiguous array makes a copy, and the caller's buffer would stay empty)
        if not isinstance(out, np.ndarray) or out.dtype != dt or out.size != n * per_out or not out.flags.c_contiguous:
            raise DabGpuError("chain: output buffer does not match (dtype %s, %d elements, C-contiguous)" % (dt, n * per_out))
        flat = out.reshape(-1)
        assert flat.size == 0 or np.shares_memory(flat, out)
        out = flat
        ob = C.c_size_t()
        self._chk(self._lib.dabgpu_chain_process(self._h, bits.ctypes.data, n, stages,
                                                 out.ctypes.data, out.nbytes, C.byref(ob)))
        return out.reshape(n, per_out)

    # ---- the front-end on the device: ETI(NI) frames -> coded bits -> IQ (include/dabgpu.h) ----
    @staticmethod
    def _eti(eti):
        eti = np.ascontiguousarray(eti, np.uint8).reshape(-1)
        if eti.size % ETI_FRAME_BYTES:
            raise DabGpuError("frontend: ETI frames are 6144 bytes")
        return eti, eti.size // ETI_FRAME_BYTES

    @staticmethod
    def frontend_describe(frame):
        """The layout of one raw ETI(NI) frame (host only: needs the library, no device): a dictionary of mode, fic_bytes,
        fic_offset, fic_rules [(groups, pattern)], tail (bytes, pattern), nst and, per sub-channel in STC order, sad, stl,
        tpl, framesize, cu, padding_byte, offset, rules.  Raises DabGpuError with the message of the CPU class that refuses
        the frame."""
        lib = load_library()
        frame = np.ascontiguousarray(frame, np.uint8).reshape(-1)
        if frame.size != ETI_FRAME_BYTES:
            raise DabGpuError("frontend: ETI frames are 6144 bytes")
        lay = _FeLayout()
        if lib.dabgpu_frontend_describe(frame.ctypes.data, C.byref(lay)) != 0:
            raise DabGpuError(lib.dabgpu_last_error(None).decode())
        rules = lambda r, n: [(int(r[i].groups), int(r[i].pattern)) for i in range(n)]  # noqa: E731
        subs = []
        for i in range(lay.nst):
            s = lay.sub[i]
            d = {k: int(getattr(s, k)) for k in ("sad", "stl", "tpl", "framesize", "cu", "padding_byte", "offset")}
            d["rules"] = rules(s.rule, s.n_rules)
            subs.append(d)
        return {"mode": int(lay.mode), "fic_bytes": int(lay.fic_bytes), "fic_offset": int(lay.fic_offset),
                "fic_rules": rules(lay.fic_rule, lay.fic_n_rules), "tail": (int(lay.tail_bytes), int(lay.tail_pattern)),
                "nst": int(lay.nst), "subchannels": subs}

    def frontend_configure(self, frame):
        """Layout from one ETI frame (the stream's first, FP = 0: finding it is the caller's), zero history.  Waits."""
        frame = np.ascontiguousarray(frame, np.uint8).reshape(-1)
        if frame.size != ETI_FRAME_BYTES:
            raise DabGpuError("frontend: ETI frames are 6144 bytes")
        self._chk(self._lib.dabgpu_frontend_configure(self._h, frame.ctypes.data))
        self._fe_frame = frame.copy()                    # (dabplus_subchannels: the configured layout)

    def frontend_reset(self):
        """Zero history (the start of a stream), layout kept.  Waits."""
        self._chk(self._lib.dabgpu_frontend_reset(self._h))

    def eti_to_bits(self, eti):
        """Host path: whole transmission frames of ETI (n x 6144 uint8) -> (n_tf x tf_input_bytes) coded bits."""
        eti, n = self._eti(eti)
        per = self.geometry["tf_input_bytes"]
        out = np.empty(max(n // CIFS_PER_FRAME[self.geometry["mode"]], 1) * per, np.uint8)
        ob = C.c_size_t()
        self._chk(self._lib.dabgpu_frontend_process(self._h, eti.ctypes.data, n, out.ctypes.data, out.nbytes, C.byref(ob)))
        return out[:ob.value].reshape(-1, per)

    def eti_to_bits_dev(self, d_eti, n_eti, d_bits, stream=None):
        """Device path on torch uint8 tensors, asynchronous on the stream (as chain_dev).  The frames are not looked at."""
        s = self._stream_handle(d_eti, stream)
        ob = C.c_size_t()
        self._chk(self._lib.dabgpu_frontend_process_dev(self._h, d_eti.data_ptr(), n_eti, d_bits.data_ptr(),
                                                        d_bits.numel() * d_bits.element_size(), C.byref(ob), s))
        if not s:
            self.synchronize()
        return ob.value

    def chain_eti(self, eti, stages, out=None):
        """Host path, ETI in, IQ out (chain() with the front-end in front; the coded bits stay on the device)."""
        eti, n = self._eti(eti)
        cifs = CIFS_PER_FRAME[self.geometry["mode"]]
        n_tf = n // cifs
        dt = np.dtype(getattr(self, "_out_dtype", np.complex64))
        per_out = self.out_bytes_per_frame(stages) // dt.itemsize
        if out is None:
            out = np.empty(n_tf * per_out, dt)
        if not isinstance(out, np.ndarray) or out.dtype != dt or out.size != n_tf * per_out or not out.flags.c_contiguous:
            raise DabGpuError("chain: output buffer does not match (dtype %s, %d elements, C-contiguous)" % (dt, n_tf * per_out))
        flat = out.reshape(-1)
        ob = C.c_size_t()
        self._chk(self._lib.dabgpu_chain_process_eti(self._h, eti.ctypes.data, n, stages, flat.ctypes.data, flat.nbytes,
                                                     C.byref(ob)))
        return flat.reshape(n_tf, per_out)

    def submit_eti(self, eti, stages):
        """Asynchronous host path from ETI frames (at most two batches in flight; collect() as for submit())."""
        eti, n = self._eti(eti)
        self._chk(self._lib.dabgpu_chain_submit_eti(self._h, eti.ctypes.data, n, stages))

    # ---- front-end stream state: the time interleaver's history (include/dabgpu.h, "front-end stream state") ----
    def frontend_state(self):
        """The time interleaver's history after everything queued on the context so far, as the self-describing blob of
        dabgpu_frontend_get_state (bytes).  Waits for the context.  A whole ETI-fed stream is this blob AND stream_state()."""
        cap = self._lib.dabgpu_frontend_state_bytes(self._h)
        buf = C.create_string_buffer(cap)
        n = C.c_size_t()
        self._chk(self._lib.dabgpu_frontend_get_state(self._h, buf, cap, C.byref(n)))
        return buf.raw[:n.value]

    def set_frontend_state(self, blob):
        """Install a blob of frontend_state(), taken on a context of the same mode and multiplex layout.  Waits."""
        blob = bytes(blob)
        self._chk(self._lib.dabgpu_frontend_set_state(self._h, blob, len(blob)))

    def frontend_seed(self, eti, e):
        """The history in front of ETI frame `e` of a stream from the min(e, 15) frames before it (host array, in stream
        order; None or empty with e = 0, the start of a stream): dabgpu_frontend_seed.  No output."""
        eti, n = self._eti(eti if eti is not None else np.empty(0, np.uint8))
        self._chk(self._lib.dabgpu_frontend_seed(self._h, eti.ctypes.data if n else None, n, int(e)))

    def seed_eti(self, eti, stages, e):
        """Front-end AND chain in the state in front of ETI frame `e` (a multiple of the frames per transmission frame), from
        the min(e, 15 + that count) frames before it (streams.eti_leadin): dabgpu_chain_seed_eti.  No output."""
        eti, n = self._eti(eti if eti is not None else np.empty(0, np.uint8))
        self._chk(self._lib.dabgpu_chain_seed_eti(self._h, eti.ctypes.data if n else None, n, stages, int(e)))

    def seed_eti_dev(self, d_eti, n_leadin, stages, e, stream=None, queued=False):
        """Same with the lead-in frames in device memory (a torch uint8 tensor, or None with e = 0), asynchronous on the
        stream -- a HIP stream handle as for chain_dev, torch's current stream by default; queued=True: the context's own
        stream, in order with the queued calls that follow, without waiting for the device.  The frames are not looked at."""
        import torch
        if d_eti is not None and d_eti.numel() != n_leadin * ETI_FRAME_BYTES:
            raise DabGpuError("seed: the lead-in is n_leadin ETI frames of 6144 bytes")
        if queued:
            s = None
        else:
            where = d_eti if d_eti is not None else torch.empty(0, device=torch.device("cuda", self.device))
            s = self._stream_handle(where, stream)
        self._chk(self._lib.dabgpu_chain_seed_eti_dev(self._h, d_eti.data_ptr() if d_eti is not None and n_leadin else None,
                                                      n_leadin, stages, int(e), s))
        if not s and not queued:
            self.synchronize()

    def submit(self, bits, stages):
        """Asynchronous host path: queue a batch (at most two in flight)."""
        bits = np.ascontiguousarray(bits, np.uint8).reshape(-1)
        per = self.geometry["tf_input_bytes"]
        if bits.size % per:
            raise DabGpuError("chain: input size not valid")
        self._chk(self._lib.dabgpu_chain_submit(self._h, bits.ctypes.data, bits.size // per, stages))

    def collect(self, copy=True):
        """Wait for the oldest batch: complex64 samples (a view of the context's pinned buffer when
        copy=False: valid until the second next submit)."""
        p, n = C.c_void_p(), C.c_size_t()
        self._chk(self._lib.dabgpu_chain_collect(self._h, C.byref(p), C.byref(n)))
        dt = np.dtype(getattr(self, "_out_dtype", np.complex64))
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,)).view(dt)
        return a.copy() if copy else a

    def _stream_handle(self, tensor, stream):
        """HIP stream handle to launch on.  A real torch stream is used as is
        (fully asynchronous).  torch's legacy default stream has handle 0, which
        the C-ABI reads as "the context's own stream": in that case order the two
        by hand (drain torch's stream now, the context's stream after the call)."""
        import torch
        h = torch.cuda.current_stream(tensor.device).cuda_stream if stream is None else stream
        if not h:
            torch.cuda.current_stream(tensor.device).synchronize()
        return h

    def _dev_call(self, fn, tensor, stream, *args, queued=False):
        """The tail of a device wrapper of the receive-side stages: fn(handle, *args, stream handle), ordered as
        _stream_handle describes.  queued=True: the context's OWN stream (stream argument NULL) whatever torch's current
        stream is, returning at once -- behind every chain call queued on the context before it, whichever lane that call went
        to, and in front of the chain calls queued after it (as chain_dev_queued and post_process_dev_queued are ordered);
        torch's stream is not touched and nothing is waited for."""
        if queued:
            self._chk(fn(self._h, *args, None))
            return
        s = self._stream_handle(tensor, stream)
        self._chk(fn(self._h, *args, s))
        if not s:
            self.synchronize()

    def chain_dev(self, d_bits, n_frames, stages, d_out, stream=None):
        """Device path on torch tensors (coded bits -> IQ)."""
        s = self._stream_handle(d_bits, stream)
        ob = C.c_size_t()
        self._chk(self._lib.dabgpu_chain_process_dev(
            self._h, d_bits.data_ptr(), n_frames, stages, d_out.data_ptr(),
            d_out.numel() * d_out.element_size(), C.byref(ob), s))
        if not s:
            self.synchronize()
        return ob.value

    def symbols_dev(self, d_carriers, n_frames, stages, d_out, stream=None):
        """Device path on torch tensors (SignalMultiplexer output -> IQ)."""
        s = self._stream_handle(d_carriers, stream)
        ob = C.c_size_t()
        self._chk(self._lib.dabgpu_symbols_process_dev(
            self._h, d_carriers.data_ptr(), n_frames, stages, d_out.data_ptr(),
            d_out.numel() * d_out.element_size(), C.byref(ob), s))
        if not s:
            self.synchronize()
        return ob.value

    # ---- the receiver: native-rate IQ -> coded bits, per-frame MER and bit errors (include/dabgpu.h, "the receiver") ----
    @staticmethod
    def _iq_format(dtype):
        if dtype == np.complex64:
            return 0
        if dtype == np.int16:
            return FORMATS["s16"][0]
        raise DabGpuError("demod: input is complex64 or int16 (interleaved re, im)")

    def demod(self, iq, early=0, ref_bits=None, want_bits=True):
        """Host path: whole transmission frames of native-rate IQ (complex64, or int16 interleaved re, im) -> the coded bits
        (n_frames x tf_input_bytes uint8; None with want_bits=False).  ref_bits: bits to count the errors against.  The
        per-frame figures are monitor_stats(frame)."""
        iq = np.ascontiguousarray(iq)
        fmt = self._iq_format(iq.dtype)
        per = self.geometry["tf_samples"] * (2 if fmt else 1)
        if iq.size == 0 or iq.size % per:
            raise DabGpuError("demod: input size not valid (whole transmission frames at the native rate)")
        n = iq.size // per
        nb = self.geometry["tf_input_bytes"]
        out = np.empty((n, nb), np.uint8) if want_bits else None
        ref = None
        if ref_bits is not None:
            ref = np.ascontiguousarray(ref_bits, np.uint8).reshape(-1)
            if ref.size != n * nb:
                raise DabGpuError("demod: reference bits do not match the frames")
        self._chk(self._lib.dabgpu_demod(self._h, iq.ctypes.data, fmt, n, int(early),
                                         out.ctypes.data if want_bits else None, ref.ctypes.data if ref is not None else None))
        return out

    def demod_dev(self, d_iq, n_frames, early=0, d_bits_out=None, d_ref_bits=None, stream=None, queued=False):
        """Device path on torch tensors (complex64, or int16 pairs), asynchronous on the stream as chain_dev; d_bits_out
        (uint8, n_frames x tf_input_bytes) and d_ref_bits may be None.  queued=True, here and in every receive-side *_dev
        wrapper below: on the context's own stream without waiting, behind the chain calls queued before it (_dev_call)."""
        import torch
        fmt = 0 if d_iq.dtype == torch.complex64 else (FORMATS["s16"][0] if d_iq.dtype == torch.int16 else -1)
        if fmt < 0:
            raise DabGpuError("demod: input is complex64 or int16 (interleaved re, im)")
        if d_iq.numel() != n_frames * self.geometry["tf_samples"] * (2 if fmt else 1):
            raise DabGpuError("demod: input size not valid (whole transmission frames at the native rate)")
        for tns in (d_bits_out, d_ref_bits):
            if tns is not None and tns.numel() * tns.element_size() != n_frames * self.geometry["tf_input_bytes"]:
                raise DabGpuError("demod: bit buffers are n_frames x tf_input_bytes")
        self._dev_call(self._lib.dabgpu_demod_dev, d_iq, stream, d_iq.data_ptr(), fmt, n_frames, int(early),
                       d_bits_out.data_ptr() if d_bits_out is not None else None,
                       d_ref_bits.data_ptr() if d_ref_bits is not None else None, queued=queued)

    def demod_soft(self, iq, early=0, ref_bits=None, want_bits=False, _entry=None):
        """demod() with soft output: -> soft (n_frames x 8 tf_input_bytes int8; soft 8 p + b belongs to bit 0x80 >> b of byte
        p, > 0: more likely 1, a clean flat symbol gives +-64), or (soft, bits) with want_bits=True.  The per-frame figures
        are monitor_stats(frame), as after demod()."""
        iq = np.ascontiguousarray(iq)
        fmt = self._iq_format(iq.dtype)
        per = self.geometry["tf_samples"] * (2 if fmt else 1)
        if iq.size == 0 or iq.size % per:
            raise DabGpuError("demod: input size not valid (whole transmission frames at the native rate)")
        n = iq.size // per
        nb = self.geometry["tf_input_bytes"]
        soft = np.empty((n, 8 * nb), np.int8)
        out = np.empty((n, nb), np.uint8) if want_bits else None
        ref = None
        if ref_bits is not None:
            ref = np.ascontiguousarray(ref_bits, np.uint8).reshape(-1)
            if ref.size != n * nb:
                raise DabGpuError("demod: reference bits do not match the frames")
        self._chk((_entry or self._lib.dabgpu_demod_soft)(self._h, iq.ctypes.data, fmt, n, int(early), soft.ctypes.data,
                                                          out.ctypes.data if want_bits else None, ref.ctypes.data if ref is not None else None))
        return (soft, out) if want_bits else soft

    def demod_soft_dev(self, d_iq, n_frames, d_soft_out, early=0, d_bits_out=None, d_ref_bits=None, stream=None, queued=False,
                       _entry=None):
        """demod_dev() with soft output: d_soft_out is int8, n_frames x 8 tf_input_bytes."""
        import torch
        fmt = 0 if d_iq.dtype == torch.complex64 else (FORMATS["s16"][0] if d_iq.dtype == torch.int16 else -1)
        if fmt < 0:
            raise DabGpuError("demod: input is complex64 or int16 (interleaved re, im)")
        if d_iq.numel() != n_frames * self.geometry["tf_samples"] * (2 if fmt else 1):
            raise DabGpuError("demod: input size not valid (whole transmission frames at the native rate)")
        if d_soft_out is None or d_soft_out.numel() * d_soft_out.element_size() != 8 * n_frames * self.geometry["tf_input_bytes"]:
            raise DabGpuError("demod: the soft buffer is n_frames x 8 tf_input_bytes int8")
        for tns in (d_bits_out, d_ref_bits):
            if tns is not None and tns.numel() * tns.element_size() != n_frames * self.geometry["tf_input_bytes"]:
                raise DabGpuError("demod: bit buffers are n_frames x tf_input_bytes")
        self._dev_call(_entry or self._lib.dabgpu_demod_soft_dev, d_iq, stream, d_iq.data_ptr(), fmt, n_frames, int(early),
                       d_soft_out.data_ptr(), d_bits_out.data_ptr() if d_bits_out is not None else None,
                       d_ref_bits.data_ptr() if d_ref_bits is not None else None, queued=queued)

    # ---- the carrier state: weighted softs, MER per carrier (include/dabgpu.h, "the carrier state") ----
    def demod_csi(self, iq, early=0, ref_bits=None, want_bits=False):
        """demod_soft() with every metric weighted by the state of its carrier, measured on the frame itself (A_k / V_k,
        normalised to 1 on white noise): the same arguments, layout, bits and per-frame figures.  carrier_state(frame) reads
        what the weights were formed from."""
        return self.demod_soft(iq, early, ref_bits, want_bits, _entry=self._lib.dabgpu_demod_csi)

    def demod_csi_dev(self, d_iq, n_frames, d_soft_out, early=0, d_bits_out=None, d_ref_bits=None, stream=None, queued=False):
        """demod_soft_dev() with weighted metrics; queued=True as there."""
        self.demod_soft_dev(d_iq, n_frames, d_soft_out, early, d_bits_out, d_ref_bits, stream, queued,
                            _entry=self._lib.dabgpu_demod_csi_dev)

    def demod_carrier_state(self, iq, early=0):
        """The carrier state and the weights alone (host path, whole frames as demod() takes them): the per-carrier MER
        readout.  -> the number of frames; read them with carrier_state(frame)."""
        iq = np.ascontiguousarray(iq)
        fmt = self._iq_format(iq.dtype)
        per = self.geometry["tf_samples"] * (2 if fmt else 1)
        if iq.size == 0 or iq.size % per:
            raise DabGpuError("demod: input size not valid (whole transmission frames at the native rate)")
        self._chk(self._lib.dabgpu_demod_carrier_state(self._h, iq.ctypes.data, fmt, iq.size // per, int(early)))
        return iq.size // per

    def demod_carrier_state_dev(self, d_iq, n_frames, early=0, stream=None, queued=False):
        """demod_carrier_state() on a torch tensor (complex64, or int16 pairs), asynchronous on the stream as demod_dev."""
        import torch
        fmt = 0 if d_iq.dtype == torch.complex64 else (FORMATS["s16"][0] if d_iq.dtype == torch.int16 else -1)
        if fmt < 0:
            raise DabGpuError("demod: input is complex64 or int16 (interleaved re, im)")
        if d_iq.numel() != n_frames * self.geometry["tf_samples"] * (2 if fmt else 1):
            raise DabGpuError("demod: input size not valid (whole transmission frames at the native rate)")
        self._dev_call(self._lib.dabgpu_demod_carrier_state_dev, d_iq, stream, d_iq.data_ptr(), fmt, n_frames, int(early),
                       queued=queued)

    def carrier_state(self, frame=0):
        """Frame `frame` of the most recent demod_csi*() / demod_carrier_state*() (waits for it): A, V (int64, the raw
        fixed-point sums per carrier position), w (float32, the weights) and mer_db per carrier
        (20 log10(A / sqrt(2^(CSI_FRAC_BITS - 1) S V)), S = nb_symbols - 1; inf where V = 0)."""
        K = self.geometry["carriers"]
        A, V, w = np.empty(K, np.int64), np.empty(K, np.int64), np.empty(K, np.float32)
        self._chk(self._lib.dabgpu_get_carrier_state(self._h, frame, A.ctypes.data, V.ctypes.data, w.ctypes.data))
        S = self.geometry["nb_symbols"] - 1
        with np.errstate(divide="ignore", invalid="ignore"):
            mer = 20.0 * np.log10(A.astype(np.float64) / np.sqrt(2.0 ** (CSI_FRAC_BITS - 1) * S * V.astype(np.float64)))
        return {"A": A, "V": V, "w": w, "mer_db": mer}

    def set_csi_unit_weights(self, enable):
        """Diagnostic: every weight 1 (demod_csi() then writes demod_soft()'s bytes)."""
        self._chk(self._lib.dabgpu_debug_csi_unit_weights(self._h, int(bool(enable))))

    def set_monitor(self, enable, early=-1):
        """Demodulate every native-rate chain call's output against its own coded bits (off by default); early < 0: from
        the call's filter and window.  The figures: monitor_stats(frame)."""
        self._chk(self._lib.dabgpu_set_monitor(self._h, int(bool(enable)), int(early)))

    def monitor_stats(self, frame=0):
        """Frame `frame` of the most recent demod() / demod_dev() or monitored chain call (waits for it): sum_signal,
        sum_quadrature, bit_errors, n_bits, min_margin, and mer_db = 10 log10(sum_signal / sum_quadrature)."""
        st = _DemodStats()
        self._chk(self._lib.dabgpu_get_demod_stats(self._h, frame, C.byref(st)))
        d = {k: getattr(st, k) for k, _ in _DemodStats._fields_}
        d["bit_errors"], d["n_bits"] = int(d["bit_errors"]), int(d["n_bits"])
        with np.errstate(divide="ignore", invalid="ignore"):
            d["mer_db"] = float(10.0 * np.log10(np.float64(st.sum_signal) / np.float64(st.sum_quadrature)))
        return d

    def set_demod_run_symbols(self, symbols=0):
        """Diagnostic: data symbols per workgroup of the receiver's kernel (0: chosen from the batch size)."""
        self._chk(self._lib.dabgpu_debug_demod_run_symbols(self._h, int(symbols)))

    # ---- the synchroniser: frame starts and carrier offset of a capture (include/dabgpu.h, "the synchroniser") ----
    # (the capture helpers below serve every stage that takes one: `stage` starts their refusals)
    @staticmethod
    def _capture_host(stage, iq):
        """-> (the capture as a flat contiguous array, its format, its samples)"""
        iq = np.ascontiguousarray(iq)
        if iq.dtype == np.complex64:
            return iq.reshape(-1), 0, iq.size
        if iq.dtype == np.int16 and iq.size % 2 == 0:
            return iq.reshape(-1), FORMATS["s16"][0], iq.size // 2
        raise DabGpuError(stage + ": input format is complex64 or int16 (interleaved re, im)")

    @staticmethod
    def _capture_tensor(stage, d_iq):
        """-> (the tensor's format, its samples)"""
        import torch
        if d_iq.dtype == torch.complex64:
            return 0, d_iq.numel()
        if d_iq.dtype == torch.int16 and d_iq.numel() % 2 == 0:
            return FORMATS["s16"][0], d_iq.numel() // 2
        if d_iq.dtype in (torch.uint8, torch.int8):
            return FORMATS["u8" if d_iq.dtype == torch.uint8 else "s8"][0], d_iq.numel() // 2      # (the library refuses them)
        raise DabGpuError(stage + ": input format is complex64 or int16 (interleaved re, im)")

    def _frames_host(self, stage, frames):
        """A host capture of whole transmission frames -> (flat array, format, frames)"""
        iq, fmt, n = self._capture_host(stage, frames)
        tf = self.geometry["tf_samples"]
        if n % tf:
            raise DabGpuError(stage + ": the input is whole transmission frames (tf_samples each)")
        return iq, fmt, n // tf

    def _frames_tensor(self, stage, d_frames, n_frames):
        """A contiguous tensor that holds n_frames whole transmission frames -> its format"""
        fmt, n = self._capture_tensor(stage, d_frames)
        if int(n_frames) < 0 or n < int(n_frames) * self.geometry["tf_samples"] or not d_frames.is_contiguous():
            raise DabGpuError(stage + ": the tensor is contiguous and holds n_frames whole transmission frames")
        return fmt

    def sync_slots(self, n_samples):
        """Frames an extraction of an n_samples capture writes: min(max_frames, n_samples // tf_samples)."""
        return min(self.max_frames, int(n_samples) // self.geometry["tf_samples"])

    def sync(self, iq, max_shift=31):
        """Host path: a native-rate capture (complex64, or int16 interleaved re, im) -> sync_result()."""
        iq, fmt, n = self._capture_host("sync", iq)
        self._chk(self._lib.dabgpu_sync(self._h, iq.ctypes.data, fmt, n, int(max_shift)))
        return self.sync_result()

    def sync_dev(self, d_iq, max_shift=31, stream=None, queued=False):
        """Device path on a torch tensor (complex64, or int16 pairs), asynchronous on the stream as chain_dev; the records
        are sync_result(), the frames sync_extract_dev()."""
        fmt, n = self._capture_tensor("sync", d_iq)
        self._dev_call(self._lib.dabgpu_sync_dev, d_iq, stream, d_iq.data_ptr(), fmt, n, int(max_shift), queued=queued)

    def sync_result(self):
        """The candidate frames of the most recent sync() / sync_dev() (waits for it): a list of dicts start, shift, valid, eps,
        cfo_hz, quality, null_depth.  Near eps = +-1/2 only shift + eps is meaningful."""
        n = C.c_size_t()
        cap = max(self.max_frames, 1)
        recs = (_SyncFrame * cap)()
        self._chk(self._lib.dabgpu_get_sync_result(self._h, C.byref(n), recs, cap))
        return [{k: getattr(recs[i], k) for k, _ in _SyncFrame._fields_} for i in range(min(n.value, cap))]

    def sync_result_bytes(self):
        """The same records as the bytes the device wrote (n_frames x 48)."""
        n = C.c_size_t()
        cap = max(self.max_frames, 1)
        recs = (_SyncFrame * cap)()
        self._chk(self._lib.dabgpu_get_sync_result(self._h, C.byref(n), recs, cap))
        return bytes(recs)[:min(n.value, cap) * C.sizeof(_SyncFrame)]

    def sync_extract(self, iq):
        """Host path: the capture the most recent sync() was given -> (sync_slots, tf_samples) complex64, every valid frame
        rotated back by its offset and cut out at its start; frames that are not valid are zeros."""
        iq, fmt, n = self._capture_host("sync", iq)
        out = np.empty((self.sync_slots(n), self.geometry["tf_samples"]), np.complex64)
        self._chk(self._lib.dabgpu_sync_extract(self._h, iq.ctypes.data, fmt, n, out.ctypes.data))
        return out

    def sync_extract_dev(self, d_iq, d_frames_out, stream=None, queued=False):
        """Device path: d_frames_out is complex64, sync_slots(n_samples) x tf_samples."""
        import torch
        fmt, n = self._capture_tensor("sync", d_iq)
        if d_frames_out.dtype != torch.complex64 or d_frames_out.numel() != self.sync_slots(n) * self.geometry["tf_samples"]:
            raise DabGpuError("sync_extract: the output is complex64, sync_slots(n_samples) x tf_samples")
        self._dev_call(self._lib.dabgpu_sync_extract_dev, d_iq, stream, d_iq.data_ptr(), fmt, n, d_frames_out.data_ptr(), queued=queued)

    # ---- the channel emulator: paths, Doppler and seeded noise on a sample stream (include/dabgpu.h, "the channel") ----
    def set_channel(self, paths, sigma=0.0, seed=0, rate_hz=2048000.0):
        """Install a channel: paths are (delay, gain, doppler_hz) tuples, the gain complex; sigma is absolute, per component
        (channel_sigma).  History and position stay; takes effect at the next call."""
        cfg = _channel_config(paths, sigma, seed, rate_hz)
        self._chk(self._lib.dabgpu_set_channel(self._h, C.byref(cfg)))

    def channel_reset(self, position=0):
        """Zero history; the stream continues at `position`."""
        self._chk(self._lib.dabgpu_channel_reset(self._h, int(position) & (2 ** 64 - 1)))

    def channel_position(self):
        """Samples the stream has taken since the last reset, plus the reset's position (waits for the most recent call)."""
        pos = C.c_uint64()
        self._chk(self._lib.dabgpu_get_channel_position(self._h, C.byref(pos)))
        return int(pos.value)

    def set_channel_run_samples(self, samples=0):
        """Diagnostic: samples per workgroup of the channel's kernel (0: chosen from the call size)."""
        self._chk(self._lib.dabgpu_debug_channel_run_samples(self._h, int(samples)))

    def channel(self, iq, out="complexf"):
        """Host path: the next samples of the stream (complex64, or int16 interleaved re, im) through the channel ->
        complex64, or int16 pairs with out="s16"."""
        iq, fmt, n = self._capture_host("channel", iq)
        if out not in ("complexf", "s16"):
            raise DabGpuError("channel: formats are complexf (0) or DABGPU_FMT_S16")
        y = np.empty(n, np.complex64) if out == "complexf" else np.empty(2 * n, np.int16)
        # (an empty array has no buffer worth the name: the library refuses n_samples = 0 on whatever pointer it gets)
        self._chk(self._lib.dabgpu_channel(self._h, iq.ctypes.data, fmt, n, y.ctypes.data, 0 if out == "complexf" else FORMATS["s16"][0]))
        return y

    def channel_dev(self, d_in, d_out, stream=None, queued=False):
        """Device path on torch tensors (complex64, or int16 pairs; contiguous, the same number of samples), asynchronous on
        the stream as chain_dev."""
        import torch
        for t in (d_in, d_out):
            if t.dtype not in (torch.complex64, torch.int16) or (t.dtype == torch.int16 and t.numel() % 2):
                raise DabGpuError("channel: tensors are complex64 or int16 (interleaved re, im)")
        fi, n = self._capture_tensor("channel", d_in)
        fo, m = self._capture_tensor("channel", d_out)
        if n != m or not d_in.is_contiguous() or not d_out.is_contiguous():
            raise DabGpuError("channel: input and output are contiguous and hold the same number of samples")
        self._dev_call(self._lib.dabgpu_channel_dev, d_in, stream, d_in.data_ptr(), fi, n, d_out.data_ptr(), fo, queued=queued)

    # ---- the clock: a sampling-clock offset put on a sample stream, or taken off it (include/dabgpu.h, "the clock") ----
    def set_clock(self, ppm):
        """Install a clock offset in ppm (|ppm| <= 1000); implies clock_reset(0).  Takes effect at the next call."""
        self._chk(self._lib.dabgpu_set_clock(self._h, float(ppm)))

    def clock_reset(self, position=0):
        """Zero history; the stream continues at input sample `position`, the output at clock_count(ppm, position)."""
        if not 0 <= int(position) < 2 ** 64:
            raise DabGpuError("clock: the stream's position must not exceed 2^62")
        self._chk(self._lib.dabgpu_clock_reset(self._h, int(position)))

    def clock_position(self):
        """Input samples the stream has taken since the last reset, plus the reset's position (waits for the most recent call)."""
        pos = C.c_uint64()
        self._chk(self._lib.dabgpu_get_clock_position(self._h, C.byref(pos)))
        return int(pos.value)

    def set_clock_run_samples(self, samples=0):
        """Diagnostic: outputs per workgroup of the clock's kernel (0: the default)."""
        self._chk(self._lib.dabgpu_debug_clock_run_samples(self._h, int(samples)))

    def clock(self, iq, out="complexf"):
        """Host path: the next samples of the stream (complex64, or int16 interleaved re, im) through the clock -> the outputs
        these samples complete: complex64, or int16 pairs with out="s16"."""
        iq, fmt, n = self._capture_host("clock", iq)
        if out not in ("complexf", "s16"):
            raise DabGpuError("clock: formats are complexf (0) or DABGPU_FMT_S16")
        cap = clock_out_max(n)
        y = np.empty(cap, np.complex64) if out == "complexf" else np.empty(2 * cap, np.int16)
        got = C.c_size_t()
        self._chk(self._lib.dabgpu_clock(self._h, iq.ctypes.data, fmt, n, y.ctypes.data, 0 if out == "complexf" else FORMATS["s16"][0],
                                         cap, C.byref(got)))
        return y[:got.value if out == "complexf" else 2 * got.value].copy()

    def clock_dev(self, d_in, d_out, stream=None, queued=False):
        """Device path on torch tensors (complex64, or int16 pairs; contiguous), asynchronous on the stream as chain_dev.
        d_out's size is the capacity.  Returns the number of output samples the call writes."""
        import torch
        for t in (d_in, d_out):
            if t.dtype not in (torch.complex64, torch.int16) or (t.dtype == torch.int16 and t.numel() % 2):
                raise DabGpuError("clock: tensors are complex64 or int16 (interleaved re, im)")
        fi, n = self._capture_tensor("clock", d_in)
        fo, cap = self._capture_tensor("clock", d_out)
        if not d_in.is_contiguous() or not d_out.is_contiguous():
            raise DabGpuError("clock: input and output are contiguous")
        got = C.c_size_t()
        self._dev_call(self._lib.dabgpu_clock_dev, d_in, stream, d_in.data_ptr(), fi, n, d_out.data_ptr(), fo, cap, C.byref(got),
                       queued=queued)
        return int(got.value)

    # ---- the tuner: any capture rate and offset down to native-rate IQ (include/dabgpu.h, "the tuner") ----
    _TUNER_HOST = {np.dtype(np.complex64): 0, np.dtype(np.int16): 1, np.dtype(np.uint8): 2, np.dtype(np.int8): 3}

    def set_tuner(self, in_rate, selectivity=0, offset_hz=0.0):
        """Install a tuner setting: the capture's rate in Hz, selectivity 0 (wide) or 1 (channel), and the offset of the wanted
        block's centre in the capture; implies tuner_reset(0).  Takes effect at the next call."""
        cfg = _tuner_config(in_rate, selectivity, offset_hz)
        self._chk(self._lib.dabgpu_set_tuner(self._h, C.byref(cfg)))
        self._tuner_cfg = cfg

    def tuner_reset(self, position=0):
        """Zero history; the stream continues at input sample `position`, the output at tuner_count(..., position)."""
        if not 0 <= int(position) < 2 ** 64:
            raise DabGpuError("tuner: the stream's position must not exceed 2^50")
        self._chk(self._lib.dabgpu_tuner_reset(self._h, int(position)))

    def tuner_position(self):
        """Input samples the stream has taken since the last reset, plus the reset's position (waits for the most recent call)."""
        pos = C.c_uint64()
        self._chk(self._lib.dabgpu_get_tuner_position(self._h, C.byref(pos)))
        return int(pos.value)

    def set_tuner_run_samples(self, samples=0):
        """Diagnostic: outputs per workgroup of the tuner's kernels (0: chosen from the setting; clamped to what fits)."""
        self._chk(self._lib.dabgpu_debug_tuner_run_samples(self._h, int(samples)))

    def _tuner_out_max(self, n_in):
        cfg = getattr(self, "_tuner_cfg", None)
        if cfg is None:
            raise DabGpuError("tuner: no setting (no dabgpu_set_tuner call yet)")
        return int(self._lib.dabgpu_tuner_out_max(C.byref(cfg), int(n_in)))

    def tuner(self, x, out="complexf"):
        """Host path: the next samples of the capture (complex64, or int16 / uint8 / int8 interleaved re, im) through the tuner
        -> the native-rate outputs these samples complete: complex64, or int16 pairs with out="s16"."""
        x = np.ascontiguousarray(x).reshape(-1)
        fmt = self._TUNER_HOST.get(x.dtype)
        if fmt is None or (fmt and x.size % 2):
            raise DabGpuError("tuner: input is complex64, or int16 / uint8 / int8 (interleaved re, im)")
        if out not in ("complexf", "s16"):
            raise DabGpuError("tuner: output format is complexf (0) or DABGPU_FMT_S16")
        n = x.size if fmt == 0 else x.size // 2
        cap = self._tuner_out_max(n)
        y = np.empty(cap, np.complex64) if out == "complexf" else np.empty(2 * cap, np.int16)
        got = C.c_size_t()
        self._chk(self._lib.dabgpu_tuner(self._h, x.ctypes.data, fmt, n, y.ctypes.data, 0 if out == "complexf" else FORMATS["s16"][0],
                                         cap, C.byref(got)))
        return y[:got.value if out == "complexf" else 2 * got.value].copy()

    def tuner_dev(self, d_in, d_out, stream=None, queued=False):
        """Device path on torch tensors (input complex64, or int16 / uint8 / int8 pairs; output complex64 or int16 pairs;
        contiguous), asynchronous on the stream as chain_dev.  d_out's size is the capacity.  Returns the number of output
        samples the call writes."""
        import torch
        fi = {torch.complex64: 0, torch.int16: 1, torch.uint8: 2, torch.int8: 3}.get(d_in.dtype)
        fo = {torch.complex64: 0, torch.int16: 1}.get(d_out.dtype)
        if fi is None or (fi and d_in.numel() % 2):
            raise DabGpuError("tuner: input is complex64, or int16 / uint8 / int8 (interleaved re, im)")
        if fo is None or (fo and d_out.numel() % 2):
            raise DabGpuError("tuner: output is complex64 or int16 (interleaved re, im)")
        if not d_in.is_contiguous() or not d_out.is_contiguous():
            raise DabGpuError("tuner: input and output are contiguous")
        n = d_in.numel() if fi == 0 else d_in.numel() // 2
        cap = d_out.numel() if fo == 0 else d_out.numel() // 2
        got = C.c_size_t()
        self._dev_call(self._lib.dabgpu_tuner_dev, d_in, stream, d_in.data_ptr(), fi, n, d_out.data_ptr(), fo, cap, C.byref(got),
                       queued=queued)
        return int(got.value)

    def sco(self, frames, early=0):
        """Host path: whole transmission frames at the native rate (complex64, or int16 interleaved re, im) -> sco_result()."""
        iq, fmt, n_frames = self._frames_host("sco", frames)
        self._chk(self._lib.dabgpu_sco(self._h, iq.ctypes.data, fmt, n_frames, int(early)))

    def sco_dev(self, d_frames, n_frames, early=0, stream=None, queued=False):
        """Device path on a torch tensor (complex64, or int16 pairs) holding n_frames whole frames, asynchronous on the stream
        as chain_dev."""
        fmt = self._frames_tensor("sco", d_frames, n_frames)
        self._dev_call(self._lib.dabgpu_sco_dev, d_frames, stream, d_frames.data_ptr(), fmt, int(n_frames), int(early), queued=queued)

    def sco_result(self, frame=-1):
        """The clock estimate of the most recent sco* call (waits for it): dict(a_hi, a_lo, s, ppm, residual_cfo, quality,
        valid, raw).  frame -1: from the sums over all valid frames.  raw: the record's bytes."""
        st = _ScoFrame()
        self._chk(self._lib.dabgpu_get_sco(self._h, int(frame), C.byref(st)))
        return {"a_hi": complex(st.a_hi_re, st.a_hi_im), "a_lo": complex(st.a_lo_re, st.a_lo_im), "s": float(st.s),
                "ppm": float(st.ppm), "residual_cfo": float(st.residual_cfo), "quality": float(st.quality),
                "valid": int(st.valid), "raw": bytes(st)}

    # ---- the TII analyser: transmitters, levels and delays of whole frames (include/dabgpu.h, "the TII analyser") ----
    def tii_scan(self, frames, early, old_variant=False, min_ratio=12.0, min_rel=1e-3):
        """Host path: whole transmission frames at the native rate (complex64, or int16 interleaved re, im) ->
        tii_scan_result()."""
        iq, fmt, n_frames = self._frames_host("tii_scan", frames)
        cfg = _tii_scan_config(early, old_variant, min_ratio, min_rel)
        self._chk(self._lib.dabgpu_tii_scan(self._h, iq.ctypes.data, fmt, n_frames, C.byref(cfg)))
        return self.tii_scan_result()

    def tii_scan_dev(self, d_frames, n_frames, early, old_variant=False, min_ratio=12.0, min_rel=1e-3, stream=None, queued=False):
        """Device path on a torch tensor (complex64, or int16 pairs) that holds n_frames whole frames, asynchronous on the
        stream as chain_dev; the result: tii_scan_result()."""
        fmt = self._frames_tensor("tii_scan", d_frames, n_frames)
        cfg = _tii_scan_config(early, old_variant, min_ratio, min_rel)
        self._dev_call(self._lib.dabgpu_tii_scan_dev, d_frames, stream, d_frames.data_ptr(), fmt, int(n_frames), C.byref(cfg), queued=queued)

    def _tii_scan_raw(self):
        head, recs = _TiiScanHead(), (_TiiEntry * TII_SLOTS)()
        self._chk(self._lib.dabgpu_get_tii_scan(self._h, C.byref(head), recs, TII_SLOTS))
        return head, recs

    def tii_scan_result(self):
        """The most recent tii_scan() / tii_scan_dev() (waits for it): (head, entries) -- head: a dict n_used, parity,
        n_entries, floor, total; entries: one dict per comb with a set cell, in comb order: comb, pattern (-1: not four
        cells), mask, n_set, energy, delay_coarse, delay, runner_up.  Delays are in samples."""
        head, recs = self._tii_scan_raw()
        h = dict(n_used=head.n_used, parity=head.parity, n_entries=head.n_entries, floor=head.floor, total=list(head.total))
        return h, [{k: getattr(recs[i], k) for k, _ in _TiiEntry._fields_} for i in range(min(head.n_entries, TII_SLOTS))]

    def tii_scan_result_bytes(self):
        """The same result as the bytes the device wrote: the head (40), then 24 entry slots of 48, zeros behind n_entries."""
        head, recs = self._tii_scan_raw()
        return bytes(head) + bytes(recs)

    # ---- the channel estimator: impulse response and echoes of whole frames (include/dabgpu.h, "the channel estimator") ----
    def cir(self, frames, early, window=1, min_ratio=20.0, min_rel=1e-3):
        """Host path: whole transmission frames at the native rate (complex64, or int16 interleaved re, im) -> cir_result()."""
        iq, fmt, n_frames = self._frames_host("cir", frames)
        cfg = _cir_config(early, window, min_ratio, min_rel)
        self._chk(self._lib.dabgpu_cir(self._h, iq.ctypes.data, fmt, n_frames, C.byref(cfg)))
        return self.cir_result()

    def cir_dev(self, d_frames, n_frames, early, window=1, min_ratio=20.0, min_rel=1e-3, stream=None, queued=False):
        """Device path on a torch tensor (complex64, or int16 pairs) that holds n_frames whole frames, asynchronous on the
        stream as chain_dev; the result: cir_result(), cir_profile()."""
        fmt = self._frames_tensor("cir", d_frames, n_frames)
        cfg = _cir_config(early, window, min_ratio, min_rel)
        self._dev_call(self._lib.dabgpu_cir_dev, d_frames, stream, d_frames.data_ptr(), fmt, int(n_frames), C.byref(cfg), queued=queued)

    def _cir_raw(self):
        head, recs = _CirHead(), (_CirPath * CIR_MAX_PATHS)()
        self._chk(self._lib.dabgpu_get_cir(self._h, C.byref(head), recs, CIR_MAX_PATHS))
        return head, recs

    def cir_result(self):
        """The most recent cir() / cir_dev() (waits for it): (head, paths) -- head: a dict of the fields of dabgpu_cir_head;
        paths: one dict per reported path in descending power: index, delay, fine, power.  Delays are in samples."""
        head, recs = self._cir_raw()
        h = {k: getattr(head, k) for k, _ in _CirHead._fields_ if k != "reserved"}
        return h, [{k: getattr(recs[i], k) for k, _ in _CirPath._fields_ if k != "reserved"}
                   for i in range(min(head.n_paths, CIR_MAX_PATHS))]

    def cir_result_bytes(self):
        """The same result as the bytes the device wrote: the head (128), then 16 path slots of 32, zeros behind n_paths."""
        head, recs = self._cir_raw()
        return bytes(head) + bytes(recs)

    def cir_profile(self):
        """(pdp, resp) of the most recent cir() / cir_dev() as float64 arrays of `spacing` values: the power delay profile per
        tap and the response per bin (0 on the unoccupied bins)."""
        n = self.geometry["spacing"]
        pdp, resp = np.zeros(n, np.float64), np.zeros(n, np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self._lib.dabgpu_get_cir_profile(self._h, pdp.ctypes.data_as(dp), resp.ctypes.data_as(dp)))
        return pdp, resp

    # ---- the FIC reader: FIB CRCs, the sub-channel table, a decoder that sets itself up (include/dabgpu.h, "the FIC reader") ----
    def fic_scan(self, images, fic_offset=None):
        """Host path: (n, 6144) uint8 images -- decode()'s output or raw ETI frames -> fic_result().  fic_offset: where the FIC
        lies in every image; None: at the configured layout's offset."""
        images, n = self._eti(images)
        off = FIC_OFFSET_CONFIGURED if fic_offset is None else int(fic_offset)
        self._chk(self._lib.dabgpu_fic_scan(self._h, images.ctypes.data, n, off))
        return self.fic_result()

    def fic_scan_dev(self, d_images, n_images, fic_offset=None, stream=None, queued=False):
        """Device path on a torch uint8 tensor that holds n_images images, asynchronous on the stream as chain_dev; the result:
        fic_result(), fic_records(), fic_services()."""
        if d_images.numel() * d_images.element_size() < int(n_images) * ETI_FRAME_BYTES:
            raise DabGpuError("fic_scan: the tensor is shorter than n_images images of 6144 bytes")
        off = FIC_OFFSET_CONFIGURED if fic_offset is None else int(fic_offset)
        self._dev_call(self._lib.dabgpu_fic_scan_dev, d_images, stream, d_images.data_ptr(), int(n_images), off, queued=queued)

    def _fic_result_raw(self):
        r = _FicResult()
        self._chk(self._lib.dabgpu_get_fic_result(self._h, C.byref(r)))
        return r

    def fic_result(self):
        """The most recent fic_scan() / fic_scan_dev() (waits for it): a dict of the fields of dabgpu_fic_result; "sub": one
        dict per SubChId seen, ascending."""
        return _fic_result_dict(self._fic_result_raw())

    def fic_result_bytes(self):
        """The same result as the 4320 bytes of dabgpu_fic_result."""
        return bytes(self._fic_result_raw())

    def fic_records(self):
        """The per-FIB records of the same call as a (FIBs, 288) uint8 array: rows of dabgpu_fic_record, in stream order."""
        n = C.c_size_t()
        self._chk(self._lib.dabgpu_get_fic_records(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, FIC_RECORD_BYTES), np.uint8)
        self._chk(self._lib.dabgpu_get_fic_records(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def fic_services(self):
        """(ensemble label or None, services) of the same call, merged on the host from the records: per service sid,
        sightings, components_dropped, label (dict or None) and components [dict(id, tmid, type, primary, ca)], in order of
        first appearance."""
        n, ens = C.c_size_t(), _FicLabel()
        self._chk(self._lib.dabgpu_get_fic_services(self._h, None, 0, C.byref(n), C.byref(ens)))
        recs = (_FicService * max(n.value, 1))()
        self._chk(self._lib.dabgpu_get_fic_services(self._h, recs, n.value, C.byref(n), C.byref(ens)))
        out = []
        for i in range(n.value):
            s = recs[i]
            out.append(dict(sid=int(s.sid), sightings=int(s.sightings), components_dropped=int(s.components_dropped),
                            label=_fic_label_dict(s.label),
                            components=[{k: int(getattr(s.comp[j], k)) for k in ("id", "tmid", "type", "primary", "ca")}
                                        for j in range(s.n_components)]))
        return _fic_label_dict(ens), out

    def configure_from_fic(self):
        """fic_make_header() on the most recent fic_scan result, then frontend_configure(): the decoder set up from what the
        signal says about itself.  Zeroes the histories, as frontend_configure does.  Waits."""
        self._chk(self._lib.dabgpu_decode_configure_from_fic(self._h))
        self._fe_frame = None                            # (dabplus_subchannels: the layout is the one the FIC result gives)

    # ---- the superframe reader: DAB+ Fire code, RS(120,110), AU CRCs (include/dabgpu.h, "the superframe reader") ----
    def superframe(self, images, offset, framesize):
        """Host path: (n, 6144) uint8 images -- decode()'s output or raw ETI frames -- and one sub-channel as the (offset,
        framesize) of frontend_describe() -> (out, result): out (n - 4, 110 s) uint8, the corrected data bytes of every
        candidate; result: superframe_result()."""
        images, n = self._eti(images)
        s = int(framesize) // 24
        out = np.zeros(max(n - 4, 1) * 110 * max(s, 1), np.uint8)
        ob = C.c_size_t()
        self._chk(self._lib.dabgpu_superframe(self._h, images.ctypes.data, n, int(offset), int(framesize), out.ctypes.data,
                                              out.nbytes, C.byref(ob)))
        return out[:ob.value].reshape(n - 4, 110 * s), self.superframe_result()

    def superframe_dev(self, d_images, n_images, offset, framesize, d_out, stream=None, queued=False):
        """Device path on torch uint8 tensors (n_images images; room for (n_images - 4) x 110 s bytes), asynchronous on the
        stream as chain_dev; returns the bytes written.  The figures: superframe_result(), superframe_records()."""
        if d_images.numel() * d_images.element_size() < int(n_images) * ETI_FRAME_BYTES:
            raise DabGpuError("superframe: the tensor is shorter than n_images images of 6144 bytes")
        ob = C.c_size_t()
        self._dev_call(self._lib.dabgpu_superframe_dev, d_images, stream, d_images.data_ptr(), int(n_images), int(offset),
                       int(framesize), d_out.data_ptr(), d_out.numel() * d_out.element_size(), C.byref(ob), queued=queued)
        return ob.value

    def superframe_result(self):
        """The most recent superframe() / superframe_dev() (waits for it): a dict of the fields of dabgpu_sf_result and
        "accepted": the indices of the accepted candidates."""
        r = _SfResult()
        self._chk(self._lib.dabgpu_get_superframe_result(self._h, C.byref(r), None, 0))
        idx = np.zeros(max(r.superframes, 1), np.uint32)
        self._chk(self._lib.dabgpu_get_superframe_result(self._h, C.byref(r), idx.ctypes.data, r.superframes))
        d = {k: int(getattr(r, k)) for k in _SF_RESULT_FIELDS if k != "reserved"}
        d["accepted"] = [int(i) for i in idx[:r.superframes]]
        return d

    def superframe_records(self):
        """The per-candidate records of the same call as a (candidates, 64) uint8 array: rows of dabgpu_sf_record."""
        n = C.c_size_t()
        self._chk(self._lib.dabgpu_get_superframe_records(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, SF_RECORD_BYTES), np.uint8)
        self._chk(self._lib.dabgpu_get_superframe_records(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def dabplus_subchannels(self):
        """The DAB+ audio sub-channels of the most recent fic_scan: per component with TMId 0 and ASCTy 63 a dict of sid,
        subchid, bitrate and, from the configured layout (the sub-channel with the same start address), offset and
        framesize -- what superframe() takes.  A sub-channel the configured layout does not hold is left out."""
        res, (_, services) = self.fic_result(), self.fic_services()
        frame = getattr(self, "_fe_frame", None)
        if frame is None:                                # configured by configure_from_fic, or not at all
            frame = fic_make_header(res, self.geometry["mode"])
        lay = self.frontend_describe(frame)
        out = []
        for svc in services:
            for comp in svc["components"]:
                if comp["tmid"] != 0 or comp["type"] != 63:
                    continue
                for sub in res["sub"]:
                    if sub["subchid"] != comp["id"]:
                        continue
                    for i, t in enumerate(lay["subchannels"]):
                        if t["sad"] == sub["sad"]:
                            out.append(dict(sid=svc["sid"], subchid=sub["subchid"], bitrate=sub["bitrate"], index=i,
                                            offset=t["offset"], framesize=t["framesize"]))
        return out

    # ---- the channel decoder: coded bits -> the ETI payload (include/dabgpu.h, "the channel decoder") ----
    def _decode_host(self, call, stats, data, dtype, per, what, ref_eti):
        """decode() / decode_soft(): `per` input items per transmission frame, `what` names them in the refusal."""
        data = np.ascontiguousarray(data, dtype).reshape(-1)
        if data.size % per:
            raise DabGpuError("decode: input size not valid (whole transmission frames of %s)" % what)
        n_tf = data.size // per
        n = n_tf * CIFS_PER_FRAME[self.geometry["mode"]]
        ref = None
        if ref_eti is not None:
            ref = np.ascontiguousarray(ref_eti, np.uint8).reshape(-1)
            if ref.size != n * ETI_FRAME_BYTES:
                raise DabGpuError("decode: the reference is one 6144-byte ETI frame per output")
        out = np.empty(max(n, 1) * ETI_FRAME_BYTES, np.uint8)
        ob = C.c_size_t()
        self._chk(call(self._h, data.ctypes.data, n_tf, out.ctypes.data, out.nbytes,
                       ref.ctypes.data if ref is not None else None, C.byref(ob)))
        return out[:ob.value].reshape(n, ETI_FRAME_BYTES), [stats(i) for i in range(n)]

    def _decode_dev(self, call, d_in, n_tf, d_eti_out, d_ref_eti, stream, queued):
        """decode_dev() / decode_soft_dev()."""
        ob = C.c_size_t()
        self._dev_call(call, d_in, stream, d_in.data_ptr(), n_tf, d_eti_out.data_ptr(),
                       d_eti_out.numel() * d_eti_out.element_size(),
                       d_ref_eti.data_ptr() if d_ref_eti is not None else None, C.byref(ob), queued=queued)
        return ob.value

    def decode(self, bits, ref_eti=None):
        """Host path: whole transmission frames of coded bits (the chain's input layout) -> (eti_images, stats).  eti_images:
        (n, 6144) uint8, the decoded FIC and sub-channel payload at their places, zeros elsewhere; output i of the call
        that brings rows e ... is ETI frame e + i - 15 of the stream (decode_reference).  ref_eti: (n, 6144), counted
        against.  stats: decode_stats(i) per output."""
        return self._decode_host(self._lib.dabgpu_decode, self.decode_stats, bits, np.uint8, self.geometry["tf_input_bytes"],
                                 "coded bits", ref_eti)

    def decode_dev(self, d_bits, n_tf, d_eti_out, d_ref_eti=None, stream=None, queued=False):
        """Device path on torch uint8 tensors, asynchronous on the stream (as chain_dev); the figures: decode_stats."""
        return self._decode_dev(self._lib.dabgpu_decode_dev, d_bits, n_tf, d_eti_out, d_ref_eti, stream, queued)

    def decode_soft(self, soft, ref_eti=None):
        """decode() on soft metrics: whole transmission frames of int8 softs in demod_soft()'s layout (8 per coded byte; any
        int8, -128 counts with magnitude 128) -> (eti_images, stats), stats: decode_soft_stats(i) per output.  A stream of its
        own beside decode()'s: the two histories do not see each other."""
        return self._decode_host(self._lib.dabgpu_decode_soft, self.decode_soft_stats, soft, np.int8,
                                 8 * self.geometry["tf_input_bytes"], "soft metrics", ref_eti)

    def decode_soft_dev(self, d_soft, n_tf, d_eti_out, d_ref_eti=None, stream=None, queued=False):
        """Device path on torch tensors (int8 softs, uint8 images), asynchronous on the stream; the figures: decode_soft_stats."""
        if d_soft.numel() * d_soft.element_size() != 8 * n_tf * self.geometry["tf_input_bytes"]:
            raise DabGpuError("decode: input size not valid (whole transmission frames of soft metrics)")
        return self._decode_dev(self._lib.dabgpu_decode_soft_dev, d_soft, n_tf, d_eti_out, d_ref_eti, stream, queued)

    def decode_soft_stats(self, frame, unit=-1):
        """Output `frame` of the most recent decode_soft() / decode_soft_dev() (waits for it): valid, metric, contra_sum (always
        equal to metric), soft_sum, corrected, erasures, coded_bits, bit_errors, n_bits.  unit as decode_stats."""
        st = _DecodeSoftStats()
        self._chk(self._lib.dabgpu_get_decode_soft_stats(self._h, frame, int(unit), C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in _DecodeSoftStats._fields_}

    def decode_reset(self):
        """Zero decoder history (the start of a received stream), layout kept.  Waits."""
        self._chk(self._lib.dabgpu_decode_reset(self._h))

    def decode_stats(self, frame, unit=-1):
        """Output `frame` of the most recent decode() / decode_dev() (waits for it): valid, corrected, coded_bits,
        bit_errors, n_bits.  unit -1: the whole frame; 0: the FIC; 1 + i: sub-channel i in STC order."""
        st = _DecodeStats()
        self._chk(self._lib.dabgpu_get_decode_stats(self._h, frame, int(unit), C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in _DecodeStats._fields_}

    # ---- the spectrum monitor: Welch power spectrum of any sample buffer (include/dabgpu.h, "the spectrum monitor") ----
    def spectrum(self, iq, window=2, accumulate=False):
        """Host path: consecutive samples as numpy complex64, or int16 / uint8 / int8 interleaved (re, im), into the Welch
        sums (2048-point segments at a hop of 1024).  The result: spectrum_stats()."""
        iq = np.ascontiguousarray(iq).reshape(-1)
        fmt = {np.dtype(np.complex64): 0, np.dtype(np.int16): 1, np.dtype(np.uint8): 2, np.dtype(np.int8): 3}.get(iq.dtype)
        if fmt is None:
            raise DabGpuError("spectrum: input is complex64, or int16 / uint8 / int8 (interleaved re, im)")
        if fmt and iq.size % 2:
            raise DabGpuError("spectrum: integer input is (re, im) pairs")
        n = iq.size if fmt == 0 else iq.size // 2
        self._chk(self._lib.dabgpu_spectrum(self._h, iq.ctypes.data if n else None, fmt, n, int(window),
                                            int(bool(accumulate))))

    def spectrum_dev(self, d_iq, window=2, accumulate=False, stream=None, n_samples=None, queued=False):
        """Device path on a torch tensor (complex64, or int16 / uint8 / int8 pairs), asynchronous on the stream as
        chain_dev; n_samples: the first so many samples of the tensor (default: all of it)."""
        import torch
        fmt = {torch.complex64: 0, torch.int16: 1, torch.uint8: 2, torch.int8: 3}.get(d_iq.dtype)
        if fmt is None:
            raise DabGpuError("spectrum: input is complex64, or int16 / uint8 / int8 (interleaved re, im)")
        if not d_iq.is_contiguous():
            raise DabGpuError("spectrum: the tensor must be contiguous (consecutive samples in memory)")
        if fmt and d_iq.numel() % 2:
            raise DabGpuError("spectrum: integer input is (re, im) pairs")
        have = d_iq.numel() if fmt == 0 else d_iq.numel() // 2
        n = have if n_samples is None else int(n_samples)
        if n > have:
            raise DabGpuError("spectrum: n_samples exceeds the tensor")
        self._dev_call(self._lib.dabgpu_spectrum_dev, d_iq, stream, d_iq.data_ptr() if n else None, fmt, n, int(window),
                       int(bool(accumulate)), queued=queued)

    def set_spectrum_monitor(self, enable, window=2):
        """Every chain call's output, whatever its rate and format, goes into the Welch sums (off by default); they
        accumulate until reset_spectrum().  The figures: spectrum_stats()."""
        self._chk(self._lib.dabgpu_set_spectrum_monitor(self._h, int(bool(enable)), int(window)))

    def reset_spectrum(self):
        self._chk(self._lib.dabgpu_reset_spectrum(self._h))

    def spectrum_stats(self, rate_hz=None):
        """Waits for the most recent spectrum work: raw (sum over segments of |X_w[k]|^2, FFT order, float64), segments,
        nfft, window, sum_w2, rate_hz (the library's for monitored chain calls, else the argument, else 0),
        psd = raw / (segments sum_w2), and freqs (Hz per bin in FFT order) when the rate is known."""
        raw = np.empty(SPECTRUM_NFFT, np.float64)
        info = _SpectrumInfo()
        self._chk(self._lib.dabgpu_get_spectrum(self._h, raw.ctypes.data_as(C.POINTER(C.c_double)), C.byref(info)))
        d = {"raw": raw, "segments": int(info.segments), "nfft": int(info.nfft), "window": int(info.window),
             "sum_w2": float(info.sum_w2), "rate_hz": float(rate_hz) if rate_hz else float(info.rate_hz)}
        with np.errstate(divide="ignore", invalid="ignore"):
            d["psd"] = raw / (d["segments"] * d["sum_w2"]) if d["segments"] and d["sum_w2"] else np.zeros_like(raw)
        d["freqs"] = spectrum_freqs(d["rate_hz"]) if d["rate_hz"] else None
        return d

    def set_resampler_run_hops(self, hops=0):
        """Diagnostic: consecutive hops per workgroup of every resampler kernel (0: chosen from the call size)."""
        self._chk(self._lib.dabgpu_debug_resampler_run_hops(self._h, int(hops)))

    def resampler_last_launch(self):
        """Diagnostic: (hops per workgroup, workgroups) of the context's most recent resampler launch; (0, 0) before the first."""
        hops, grid = C.c_int(), C.c_uint()
        self._chk(self._lib.dabgpu_debug_resampler_last_launch(self._h, C.byref(hops), C.byref(grid)))
        return int(hops.value), int(grid.value)

    def set_spectrum_run_segments(self, segments=0):
        """Diagnostic: segments per workgroup of the spectrum kernel (0: chosen from the input size)."""
        self._chk(self._lib.dabgpu_debug_spectrum_run_segments(self._h, int(segments)))

    # ---- DPD measurement: tx against the amplifier's feedback capture (include/dabgpu.h, "DPD measurement") ----
    @staticmethod
    def _dpd_host_pair(tx, rx):
        tx = np.ascontiguousarray(tx).reshape(-1)
        rx = np.ascontiguousarray(rx).reshape(-1)
        fmt = {np.dtype(np.complex64): 0, np.dtype(np.int16): 1}.get(tx.dtype)
        if fmt is None or rx.dtype != np.complex64:
            raise DabGpuError("dpd: tx is complex64 or int16 (interleaved re, im), rx is complex64")
        if fmt and tx.size % 2:
            raise DabGpuError("dpd: integer input is (re, im) pairs")
        n = tx.size if fmt == 0 else tx.size // 2
        if rx.size != n:
            raise DabGpuError("dpd: tx and rx hold the same number of samples")
        return tx, rx, fmt, n

    def _dpd_dev_pair(self, d_tx, d_rx, n_samples):
        import torch
        fmt = {torch.complex64: 0, torch.int16: 1}.get(d_tx.dtype)
        if fmt is None or d_rx.dtype != torch.complex64:
            raise DabGpuError("dpd: tx is complex64 or int16 (interleaved re, im), rx is complex64")
        if not d_tx.is_contiguous() or not d_rx.is_contiguous():
            raise DabGpuError("dpd: the tensors must be contiguous")
        if fmt and d_tx.numel() % 2:
            raise DabGpuError("dpd: integer input is (re, im) pairs")
        have = min(d_tx.numel() if fmt == 0 else d_tx.numel() // 2, d_rx.numel())
        n = have if n_samples is None else int(n_samples)
        if n > have:
            raise DabGpuError("dpd: n_samples exceeds a tensor")
        return fmt, n

    def dpd_xspectrum(self, tx, rx, rx_offset=0):
        """Host path: the Welch cross-spectrum of tx (complex64 or int16 pairs) and rx (complex64), rx segments shifted by
        rx_offset.  Returns dpd_xspectrum_result()."""
        tx, rx, fmt, n = self._dpd_host_pair(tx, rx)
        self._chk(self._lib.dabgpu_dpd_xspectrum(self._h, tx.ctypes.data if n else None, fmt, rx.ctypes.data if n else None,
                                                 n, int(rx_offset)))
        return self.dpd_xspectrum_result()

    def dpd_xspectrum_dev(self, d_tx, d_rx, rx_offset=0, stream=None, n_samples=None, queued=False):
        """Device path on torch tensors, asynchronous on the stream as chain_dev; the result: dpd_xspectrum_result()."""
        fmt, n = self._dpd_dev_pair(d_tx, d_rx, n_samples)
        self._dev_call(self._lib.dabgpu_dpd_xspectrum_dev, d_tx, stream, d_tx.data_ptr() if n else None, fmt,
                       d_rx.data_ptr() if n else None, n, int(rx_offset), queued=queued)

    def dpd_xspectrum_result(self):
        """Waits: S (2048 complex128: sum of TX conj(RX), FFT order), p_tx, p_rx (float64) and the segments used."""
        S = np.empty(SPECTRUM_NFFT, np.complex128)
        pt, pr = np.empty(SPECTRUM_NFFT, np.float64), np.empty(SPECTRUM_NFFT, np.float64)
        seg = C.c_uint64()
        dp = C.POINTER(C.c_double)
        self._chk(self._lib.dabgpu_get_dpd_xspectrum(self._h, S.view(np.float64).ctypes.data_as(dp), pt.ctypes.data_as(dp),
                                                     pr.ctypes.data_as(dp), C.byref(seg)))
        return {"S": S, "p_tx": pt, "p_rx": pr, "segments": int(seg.value)}

    def dpd_align(self, tx, rx):
        """Host path: integer lag, sub-sample delay, gain and coherence of rx against tx (two cross-spectrum passes).
        Returns a dict: lag, tau, gain (complex), coherence."""
        tx, rx, fmt, n = self._dpd_host_pair(tx, rx)
        a = _DpdAlignment()
        self._chk(self._lib.dabgpu_dpd_align(self._h, tx.ctypes.data if n else None, fmt, rx.ctypes.data if n else None, n,
                                             C.byref(a)))
        return _alignment_dict(a)

    def dpd_align_dev(self, d_tx, d_rx, stream=None, n_samples=None, queued=False):
        """Device path of dpd_align; waits for the stream, because the result is host data."""
        fmt, n = self._dpd_dev_pair(d_tx, d_rx, n_samples)
        a = _DpdAlignment()
        self._chk(self._lib.dabgpu_dpd_align_dev(self._h, d_tx.data_ptr() if n else None, fmt, d_rx.data_ptr() if n else None,
                                                 n, C.byref(a), None if queued else self._stream_handle(d_tx, stream)))
        return _alignment_dict(a)

    def dpd_measure(self, tx, rx, alignment=None, peak=1.0, n_bins=64, accumulate=False):
        """Host path: the aligned amplitude-bin statistics of the pair into the context's sums (dpd_stats()).  alignment: the
        dict dpd_align returns (None: lag 0, tau 0, gain 1)."""
        tx, rx, fmt, n = self._dpd_host_pair(tx, rx)
        al = _alignment_struct(alignment)
        self._chk(self._lib.dabgpu_dpd_measure(self._h, tx.ctypes.data if n else None, fmt, rx.ctypes.data if n else None, n,
                                               None if al is None else C.byref(al), float(peak), int(n_bins),
                                               int(bool(accumulate))))

    def dpd_measure_dev(self, d_tx, d_rx, alignment=None, peak=1.0, n_bins=64, accumulate=False, stream=None, n_samples=None, queued=False):
        """Device path of dpd_measure, asynchronous on the stream as chain_dev."""
        fmt, n = self._dpd_dev_pair(d_tx, d_rx, n_samples)
        al = _alignment_struct(alignment)
        self._dev_call(self._lib.dabgpu_dpd_measure_dev, d_tx, stream, d_tx.data_ptr() if n else None, fmt,
                       d_rx.data_ptr() if n else None, n, None if al is None else C.byref(al),
                       float(peak), int(n_bins), int(bool(accumulate)), queued=queued)

    def dpd_stats(self):
        """Waits: n_bins, peak, overflow, samples_used, and per bin count, sum_tx, sum_rx, sum_phase, sum_rx2, sum_phase2
        (float64) and raw (int64, n_bins x 6: the integers the device added)."""
        st = _DpdStats()
        self._chk(self._lib.dabgpu_get_dpd_stats(self._h, C.byref(st)))
        n = int(st.n_bins)
        d = {"n_bins": n, "peak": float(st.peak), "overflow": int(st.overflow), "samples_used": int(st.samples_used),
             "count": np.array(st.count[:n], np.uint64).astype(np.int64)}
        for name in ("sum_tx", "sum_rx", "sum_phase", "sum_rx2", "sum_phase2"):
            d[name] = np.array(getattr(st, name)[:n], np.float64)
        d["raw"] = np.ctypeslib.as_array(st.raw).reshape(DPD_MAX_BINS, 6)[:n].copy()
        return d

    def reset_dpd(self):
        self._chk(self._lib.dabgpu_reset_dpd(self._h))

    def set_dpd_geometry(self, run_segments=0, tile=0):
        """Diagnostic: segments per workgroup of the cross-spectrum kernel and tx samples per workgroup of the statistics
        kernel (0: the defaults)."""
        self._chk(self._lib.dabgpu_debug_dpd_run_segments(self._h, int(run_segments)))
        self._chk(self._lib.dabgpu_debug_dpd_tile(self._h, int(tile)))

    def synchronize(self):
        """Wait for everything the context has queued, on every lane."""
        self._chk(self._lib.dabgpu_synchronize(self._h))

    # ---- batches in flight inside the context (PipelinedModCodec's idiom, src/ModPlugin.cpp:90-154) ----
    def set_lanes(self, lanes):
        """Internal HIP streams that calls on the context's own stream rotate over (1 ... 4, default 3)."""
        self._chk(self._lib.dabgpu_set_lanes(self._h, int(lanes)))

    def lanes_info(self):
        """(lanes created so far, [lane i has a hardware queue of its own])."""
        m = C.c_int()
        n = self._lib.dabgpu_debug_lanes(self._h, C.byref(m))
        if n < 0:
            raise DabGpuError(self._lib.dabgpu_last_error(self._h).decode())
        return n, [bool(m.value >> i & 1) for i in range(n)]

    def set_handover_frames(self, frames):
        """FIRFilter -> Resampler hand-over in pieces of `frames` frames through a cache-resident ring (0: one piece)."""
        self._chk(self._lib.dabgpu_set_handover_frames(self._h, int(frames)))

    def wait_for_stream(self, stream):
        """What the context queues from now on starts after what the HIP stream (handle) holds now."""
        self._chk(self._lib.dabgpu_wait_for_stream(self._h, stream))

    def stream_wait_for(self, stream):
        """What is queued on the HIP stream (handle) from now on starts after everything the context has queued."""
        self._chk(self._lib.dabgpu_stream_wait_for(self._h, stream))

    def chain_dev_queued(self, d_in, n_frames, stages, d_out, from_bits=True):
        """Device path on the context's OWN stream (the lanes): returns at once; the output is complete after
        synchronize() or, in stream order, after stream_wait_for()."""
        ob = C.c_size_t()
        fn = self._lib.dabgpu_chain_process_dev if from_bits else self._lib.dabgpu_symbols_process_dev
        self._chk(fn(self._h, d_in.data_ptr(), n_frames, stages, d_out.data_ptr(),
                     d_out.numel() * d_out.element_size(), C.byref(ob), None))
        return ob.value

    def chain_eti_dev_queued(self, d_eti, n_eti, stages, d_bits, d_out):
        """ETI frames in device memory -> IQ on the context's OWN stream, returning at once: the front-end into d_bits
        (n_eti / frames-per-transmission-frame x tf_input_bytes, the caller's scratch), the chain from there; ordered like
        chain_dev_queued, behind a seed_eti_dev(..., queued=True) before it.  The frames are not looked at."""
        ob = C.c_size_t()
        self._chk(self._lib.dabgpu_frontend_process_dev(self._h, d_eti.data_ptr(), n_eti, d_bits.data_ptr(),
                                                        d_bits.numel() * d_bits.element_size(), C.byref(ob), None))
        return self.chain_dev_queued(d_bits, n_eti // CIFS_PER_FRAME[self.geometry["mode"]], stages, d_out)

    def post_process_dev_queued(self, d_native, stages, d_out):
        """dabgpu_post_process_dev on the context's OWN stream (stream argument NULL), returning at once: ordered behind every
        chain call queued on the context before it, whichever lane that call went to."""
        ob = C.c_size_t()
        self._chk(self._lib.dabgpu_post_process_dev(self._h, d_native.data_ptr(), d_native.numel(), stages,
                                                    d_out.data_ptr(), d_out.numel() * d_out.element_size(), C.byref(ob), None))
        return ob.value

    def format_convert_dev_queued(self, d_in, fmt, d_out):
        """dabgpu_format_process_dev on the context's OWN stream, returning at once (same ordering as above)."""
        code = FORMATS.get(fmt, (0, None))[0]
        n = d_in.numel() * (2 if d_in.is_complex() else 1)
        ob = C.c_size_t()
        self._chk(self._lib.dabgpu_format_process_dev(self._h, d_in.data_ptr(), n, code, d_out.data_ptr(),
                                                      d_out.numel() * d_out.element_size(), C.byref(ob), None, None))
        return ob.value

    # ---- stream state: the resampler's halo and the TII frame parity (include/dabgpu.h, "stream state") ----
    def stream_state(self, capacity=None):
        """The stream after everything queued on the context so far, as the self-describing blob of dabgpu_get_stream_state
        (bytes).  Waits for the context.  `capacity`: the buffer to offer instead of dabgpu_stream_state_bytes()."""
        cap = self._lib.dabgpu_stream_state_bytes(self._h) if capacity is None else int(capacity)
        buf = C.create_string_buffer(max(cap, 1))
        n = C.c_size_t()
        self._chk(self._lib.dabgpu_get_stream_state(self._h, buf, cap, C.byref(n)))
        return buf.raw[:n.value]

    def set_stream_state(self, blob):
        """Install a blob of stream_state(), taken on a context with the same mode and resampling ratio.  Waits."""
        blob = bytes(blob)
        self._chk(self._lib.dabgpu_set_stream_state(self._h, blob, len(blob)))

    def seed(self, bits, stages, frame_index):
        """The state after frames 0 ... frame_index - 1 of a stream whose frame frame_index - 1 has the coded bits `bits`
        (one frame, host array; None with frame_index 0, the start of a stream): dabgpu_chain_seed.  No output."""
        p = None
        if bits is not None:
            bits = np.ascontiguousarray(bits, np.uint8).reshape(-1)
            if bits.size != self.geometry["tf_input_bytes"]:
                raise DabGpuError("seed: the lead-in is one frame of coded bits")
            p = bits.ctypes.data
        self._chk(self._lib.dabgpu_chain_seed(self._h, p, stages, int(frame_index)))

    def seed_dev(self, d_bits, stages, frame_index, stream=None, queued=False):
        """Same with the lead-in frame in device memory (a torch uint8 tensor, or None with frame_index 0), asynchronous on
        the stream -- a HIP stream handle as for chain_dev, torch's current stream by default; queued=True: the context's own
        stream (lane 0, behind and in front of the resampler chain calls queued there), without waiting for the device.  (The
        first seed after a change of the TII, filter, window or CFR settings builds the cached TII segment, as the first
        chain call would: that one waits for the context's lanes.)"""
        import torch
        if d_bits is not None and d_bits.numel() != self.geometry["tf_input_bytes"]:
            raise DabGpuError("seed: the lead-in is one frame of coded bits")
        if queued:
            s = None
        else:
            where = d_bits if d_bits is not None else torch.empty(0, device=torch.device("cuda", self.device))
            s = self._stream_handle(where, stream)
        self._chk(self._lib.dabgpu_chain_seed_dev(self._h, d_bits.data_ptr() if d_bits is not None else None, stages,
                                                  int(frame_index), s))
        if not s and not queued:
            self.synchronize()

    def post_process_dev(self, d_native, stages, d_out, stream=None):
        """cifRes -> cifPoly on a native-rate stream in device memory (stages: STAGE_RESAMPLE and / or STAGE_POLY)."""
        s = self._stream_handle(d_native, stream)
        ob = C.c_size_t()
        self._chk(self._lib.dabgpu_post_process_dev(self._h, d_native.data_ptr(), d_native.numel(), stages,
                                                    d_out.data_ptr(), d_out.numel() * d_out.element_size(), C.byref(ob), s))
        if not s:
            self.synchronize()
        return ob.value
