"""libllsm2_amd -- MI355X-native drop-in for libllsm2's layer-0 hot path.

The product is the C-ABI shared library ``libllsm2_amd.so`` (HIP kernels for
gfx950 behind the reference's own ``llsm.h`` / ``llsmrt.h`` entry points plus
the additive batch API of ``llsm_gpu.h``).  This module is only a ctypes
binding used by the tests, ``bench.py`` and Python callers; it contains no
numerics and never falls back to a CPU implementation.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LLSM_AMD_LIB", os.path.join(_HERE, "libllsm2_amd.so"))   # override: experiment builds only

fp = C.c_float
P_fp = C.POINTER(C.c_float)
P_int = C.POINTER(C.c_int)


# ---- structs of include/llsm.h (layouts are ABI) ---------------------------
class Container(C.Structure):
    _fields_ = [("members", C.POINTER(C.c_void_p)), ("destructors", C.POINTER(C.c_void_p)),
                ("copyctors", C.POINTER(C.c_void_p)), ("nmember", C.c_int)]


class HMFrame(C.Structure):
    _fields_ = [("ampl", P_fp), ("phse", P_fp), ("nhar", C.c_int)]


class NMFrame(C.Structure):
    _fields_ = [("eenv", C.POINTER(C.POINTER(HMFrame))), ("edc", P_fp), ("psd", P_fp),
                ("npsd", C.c_int), ("nchannel", C.c_int)]


class Output(C.Structure):
    _fields_ = [("ny", C.c_int), ("fs", fp), ("y", P_fp), ("y_sin", P_fp), ("y_noise", P_fp)]


class AOptions(C.Structure):
    _fields_ = [("thop", fp), ("maxnhar", C.c_int), ("maxnhar_e", C.c_int), ("npsd", C.c_int),
                ("nchannel", C.c_int), ("chanfreq", P_fp), ("lip_radius", fp),
                ("f0_refine", C.c_int), ("hm_method", C.c_int), ("rel_winsize", fp)]


class SOptions(C.Structure):
    _fields_ = [("fs", fp), ("use_iczt", C.c_int), ("use_l1", C.c_int),
                ("iczt_param_a", fp), ("iczt_param_b", fp)]


class Chunk(C.Structure):
    _fields_ = [("conf", C.POINTER(Container)), ("frames", C.POINTER(C.POINTER(Container)))]


class Layout(C.Structure):
    _fields_ = [("n_utt", C.c_int), ("total_samples", C.c_int), ("total_frames", C.c_int),
                ("total_out", C.c_int), ("maxnhar", C.c_int), ("maxnhar_e", C.c_int),
                ("npsd", C.c_int), ("nchannel", C.c_int), ("ntemplate_ext", C.c_int)]


class FlatParams(C.Structure):
    _fields_ = [("maxnhar", C.c_int), ("maxnhar_e", C.c_int), ("npsd", C.c_int), ("nchannel", C.c_int),
                ("f0", P_fp), ("nhar", P_int), ("ampl", P_fp), ("phse", P_fp), ("psd", P_fp),
                ("psdres", P_fp), ("has_psdres", P_int), ("edc", P_fp), ("nhar_e", P_int),
                ("eenv_ampl", P_fp), ("eenv_phse", P_fp)]


class FlatL1(C.Structure):
    _fields_ = [("nspec", C.c_int), ("maxnhar", C.c_int), ("rd", P_fp), ("has_rd", P_int), ("vtmagn", P_fp),
                ("vsphse", P_fp), ("nvsphse", P_int), ("pbpsyn", P_int), ("has_hm", P_int)]


class SpliceMap(C.Structure):                              # llsm_gpu_splice_map
    _fields_ = [("utt_a", P_int), ("pos_a", P_fp), ("utt_b", P_int), ("pos_b", P_fp), ("mix", P_fp)]


class F0Options(C.Structure):                             # llsm_gpu_f0_options
    _fields_ = [("fmin", fp), ("fmax", fp), ("threshold", fp), ("silence_rel", fp), ("window_extra", C.c_int),
                ("smooth", C.c_int), ("keep_cmndf", C.c_int)]


class F0TrackOptions(C.Structure):                        # llsm_gpu_f0_track_options
    _fields_ = [("cand_threshold", fp), ("unvoiced_cost", fp), ("switch_cost", fp), ("jump_cost", fp), ("octave_cost", fp)]


class AlignOptions(C.Structure):                          # llsm_gpu_align_options
    _fields_ = [("first", C.c_int), ("count", C.c_int), ("step_cost", fp), ("voicing_cost", fp)]


class SelectOptions(C.Structure):                         # llsm_gpu_select_options
    _fields_ = [("first", C.c_int), ("count", C.c_int), ("voicing_cost", fp), ("join_cost", fp), ("join_weight", fp),
                ("skip_own_utterance", C.c_int)]


# frame / conf member indices (llsm.h)
FRAME_F0, FRAME_HM, FRAME_NM, FRAME_PSDRES = 0, 1, 2, 3
FRAME_PBPEFF, FRAME_PBPSYN, FRAME_RD, FRAME_VTMAGN, FRAME_VSPHSE = 8, 9, 10, 11, 12
CONF_NSPEC, CONF_LIPRADIUS = 10, 11
CONF_NFRM, CONF_THOP, CONF_MAXNHAR, CONF_MAXNHAR_E, CONF_NPSD = 0, 1, 2, 3, 4
CONF_FNYQ, CONF_NCHANNEL, CONF_CHANFREQ = 6, 7, 8
HMPP, HMCZT = 0, 1

# flat array ids (llsm_gpu.h)
(A_X, A_F0, A_NHAR, A_AMPL, A_PHSE, A_PSD, A_PSDRES, A_EDC, A_NHAR_E, A_EENV_AMPL,
 A_EENV_PHSE, A_XRES, A_Y, A_YSIN, A_YNOISE, A_WHITE, A_HAS_PSDRES,
 A_RD, A_VTMAGN, A_VSPHSE, A_NVSPHSE, A_PBPSYN, A_HAS_HM, A_CODE, A_NARRAYS) = range(25)

_INT_ARRAYS = {A_NHAR, A_NHAR_E, A_HAS_PSDRES, A_NVSPHSE, A_PBPSYN, A_HAS_HM}

# every symbol include/*.h declares (checked by tests/test_abi.py)
EXPORTS = """
llsm_create_fp llsm_create_int llsm_create_fparray llsm_copy_fp llsm_copy_int
llsm_copy_fparray llsm_delete_fp llsm_delete_int llsm_delete_fparray llsm_fparray_length
llsm_create_container llsm_copy_container llsm_copy_container_inplace llsm_delete_container
llsm_container_get llsm_container_attach_ llsm_container_remove
llsm_create_hmframe llsm_copy_hmframe llsm_copy_hmframe_inplace llsm_delete_hmframe
llsm_hmframe_phaseshift llsm_hmframe_harpsd
llsm_create_nmframe llsm_copy_nmframe llsm_copy_nmframe_inplace llsm_delete_nmframe
llsm_create_pbpeffect llsm_copy_pbpeffect llsm_delete_pbpeffect
llsm_create_frame llsm_frame_phaseshift llsm_frame_phasesync_rps llsm_frame_checklayer0
llsm_frame_checklayer1 llsm_conf_checklayer0 llsm_conf_checklayer1 llsm_delete_output
llsm_frame_tolayer0 llsm_chunk_tolayer1 llsm_chunk_tolayer0
llsm_gpu_batch_enable_layer1 llsm_gpu_batch_tolayer1 llsm_gpu_batch_tolayer0 llsm_gpu_batch_set_maxnhar_conf
llsm_gpu_batch_set_pbpeffect llsm_chunk_to_flat_l1 llsm_flat_l1_to_chunk
llsm_refine_f0 llsm_compute_spectrogram llsm_compute_dc llsm_harmonic_peakpicking llsm_harmonic_czt
llsm_harmonic_analysis llsm_subband_energy llsm_fft_to_psd llsm_estimate_psd llsm_warp_frequency
llsm_spectral_mean llsm_spectrum_from_envelope llsm_get_fftsize llsm_synthesize_harmonic_frame
llsm_synthesize_harmonic_frame_iczt llsm_generate_white_noise llsm_generate_bandlimited_noise
llsm_lipfilter llsm_lipfilter_reim llsm_harmonic_spectrum llsm_harmonic_envelope llsm_harmonic_minphase
llsm_create_cached_glottal_model llsm_delete_cached_glottal_model llsm_spectral_glottal_fitting
llsm_smoothing_filter llsm_lfmodel_from_rd llsm_lfmodel_spectrum llsm_lfmodel_to_gfm llsm_gfm_to_lfmodel
llsm_synthesize_harmonic_frame_auto llsm_make_filtered_pulse
llsm_create_coder llsm_delete_coder llsm_coder_encode llsm_coder_decode_layer1 llsm_coder_decode_layer0
llsm_coder_dimension llsm_coder_encode_frames llsm_coder_decode_frames
llsm_create_aoptions llsm_delete_aoptions llsm_aoptions_toconf
llsm_create_soptions llsm_delete_soptions
llsm_create_chunk llsm_copy_chunk llsm_delete_chunk llsm_chunk_phasesync_rps
llsm_chunk_phasepropagate llsm_chunk_getf0 llsm_analyze llsm_synthesize
llsm_create_rtsynth_buffer llsm_delete_rtsynth_buffer llsm_rtsynth_buffer_getlatency
llsm_rtsynth_buffer_numoutput llsm_rtsynth_buffer_feed llsm_rtsynth_buffer_fetch
llsm_rtsynth_buffer_fetch_decomposed llsm_rtsynth_buffer_clear
llsm_gpu_device_count llsm_gpu_last_error llsm_gpu_create_context llsm_gpu_delete_context
llsm_gpu_context_stream llsm_gpu_synchronize llsm_gpu_set_profiling llsm_gpu_profile_only llsm_gpu_reset_profile
llsm_gpu_get_profile llsm_gpu_fft_selftest llsm_gpu_release_cached_memory llsm_gpu_create_batch llsm_gpu_delete_batch llsm_gpu_batch_layout
llsm_gpu_batch_offsets llsm_gpu_alloc_host llsm_gpu_free_host llsm_gpu_batch_upload llsm_gpu_batch_download llsm_gpu_batch_device_ptr
llsm_gpu_batch_array_bytes llsm_gpu_batch_analyze llsm_gpu_batch_synthesize
llsm_analyze_batch llsm_synthesize_batch llsm_chunk_to_flat llsm_flat_to_chunk
llsm_gpu_set_default_seed llsm_gpu_plan_index llsm_gpu_batch_set_fnyq llsm_gpu_batch_debug_plane llsm_gpu_sum_outputs llsm_gpu_set_convention llsm_gpu_get_convention llsm_gpu_set_fanout llsm_fanout_plan llsm_fanout_selftest
llsm_chunk_blob_size llsm_chunk_to_blob llsm_blob_view llsm_blob_to_chunk llsm_blob_view_l1 llsm_gpu_batch_upload_blob llsm_gpu_batch_upload_blobs
llsm_create_rtsynth_group llsm_delete_rtsynth_group llsm_rtsynth_group_getlatency
llsm_rtsynth_group_numoutput llsm_rtsynth_group_feed llsm_rtsynth_group_feed_many llsm_rtsynth_group_fetch llsm_rtsynth_group_fetch_all llsm_gpu_rt_graph llsm_gpu_rt_graph_hops llsm_gpu_rt_fused llsm_gpu_rt_direct llsm_gpu_rt_pipeline llsm_gpu_analysis_overlap llsm_slab_stats llsm_slab_trim llsm_delete_chunks llsm_gpu_release_cached_batches llsm_gpu_device_numa_node llsm_gpu_bind_thread_to_device llsm_gpu_batch_packed_words llsm_gpu_batch_download_packed llsm_gpu_batch_upload_packed llsm_gpu_batch_download_outputs llsm_gpu_batch_download_packed_block llsm_gpu_batch_upload_packed_block llsm_gpu_batch_transfer_many llsm_gpu_batch_params_layout llsm_gpu_batch_transfer_params llsm_gpu_shared_f0_tiles llsm_gpu_synth_tables llsm_gpu_pbp_real_ifft llsm_frame_compute_snr
llsm_gpu_batch_phasesync_rps llsm_gpu_batch_phasepropagate llsm_gpu_batch_retime llsm_gpu_retime_uniform_positions
llsm_gpu_batch_pitch_formant llsm_gpu_batch_splice llsm_gpu_batch_smooth llsm_gpu_join_radii
llsm_gpu_batch_enable_coder llsm_gpu_batch_coder_dimension llsm_gpu_batch_encode llsm_gpu_batch_decode
llsm_blob_bytes llsm_gpu_batch_blob_sizes llsm_gpu_batch_download_blobs llsm_gpu_batch_download_blob_block
llsm_gpu_f0_default_options llsm_gpu_f0_plan llsm_gpu_batch_estimate_f0
llsm_gpu_f0_track_default_options llsm_gpu_f0_track_check llsm_gpu_batch_track_f0
llsm_gpu_align_default_options llsm_gpu_align_check llsm_gpu_batch_align
llsm_gpu_batch_align_band llsm_gpu_align_band_min llsm_gpu_align_band_rows
llsm_gpu_batch_align_slope llsm_gpu_align_slope_rows
llsm_gpu_batch_align_band_slope llsm_gpu_align_band_slope_min llsm_gpu_align_band_slope_rows
llsm_gpu_batch_align_around llsm_gpu_align_around_rows llsm_gpu_align_around_min llsm_gpu_align_center_line
llsm_gpu_pool_frames llsm_gpu_batch_pool_code llsm_gpu_batch_align_pyramid
llsm_gpu_align_sub_rows llsm_gpu_batch_align_sub llsm_gpu_batch_align_sub_plane
llsm_gpu_select_default_options llsm_gpu_select_check llsm_gpu_batch_select llsm_gpu_batch_select_chain
""".split()

_lib = None


def load():
    """dlopen the C-ABI library (building it first if the .so is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        from . import build as _b
        _b.build()
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.llsm_gpu_last_error.restype = C.c_char_p
    L.llsm_gpu_create_context.restype = vp
    L.llsm_gpu_create_context.argtypes = [C.c_int, vp]
    L.llsm_gpu_delete_context.argtypes = [vp]
    L.llsm_gpu_context_stream.restype = vp
    L.llsm_gpu_context_stream.argtypes = [vp]
    L.llsm_gpu_synchronize.argtypes = [vp]
    L.llsm_gpu_set_profiling.argtypes = [vp, C.c_int]
    L.llsm_gpu_profile_only.argtypes = [vp, C.c_char_p]
    L.llsm_gpu_reset_profile.argtypes = [vp]
    L.llsm_gpu_get_profile.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double), P_int]
    L.llsm_gpu_fft_selftest.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.llsm_gpu_create_batch.restype = vp
    L.llsm_gpu_create_batch.argtypes = [vp, C.POINTER(AOptions), fp, C.c_int, P_int, P_int]
    L.llsm_gpu_delete_batch.argtypes = [vp]
    L.llsm_gpu_batch_layout.argtypes = [vp, C.POINTER(Layout)]
    L.llsm_gpu_batch_offsets.argtypes = [vp, P_int, P_int, P_int]
    L.llsm_gpu_batch_upload.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.llsm_gpu_batch_download.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.llsm_gpu_batch_device_ptr.restype = vp
    L.llsm_gpu_batch_device_ptr.argtypes = [vp, C.c_int]
    L.llsm_gpu_batch_array_bytes.restype = C.c_size_t
    L.llsm_gpu_batch_array_bytes.argtypes = [vp, C.c_int]
    L.llsm_gpu_batch_analyze.argtypes = [vp]
    L.llsm_gpu_batch_synthesize.argtypes = [vp, C.POINTER(SOptions), C.c_ulonglong, C.c_int]
    L.llsm_gpu_set_default_seed.argtypes = [C.c_ulonglong]
    L.llsm_gpu_batch_set_fnyq.argtypes = [vp, fp]
    try:                                                 # (an experiment build of an earlier commit -- tools/kbench.py's HEAD leg -- lacks these)
        L.llsm_gpu_batch_debug_plane.argtypes = [vp, C.c_int, vp, C.c_longlong]; L.llsm_gpu_batch_debug_plane.restype = C.c_longlong
        L.llsm_gpu_sum_outputs.argtypes = [vp, vp, vp, C.c_longlong]; L.llsm_gpu_sum_outputs.restype = None
    except AttributeError:
        if "LLSM_AMD_LIB" not in os.environ:
            raise
    L.llsm_gpu_set_convention.argtypes = [C.c_char_p, C.c_int]
    L.llsm_gpu_get_convention.argtypes = [C.c_char_p]
    L.llsm_gpu_batch_enable_layer1.argtypes = [vp, C.c_int]
    L.llsm_gpu_batch_tolayer1.argtypes = [vp, C.c_int]
    L.llsm_gpu_batch_tolayer0.argtypes = [vp, C.c_int]
    L.llsm_gpu_batch_set_maxnhar_conf.argtypes = [vp, C.c_int]
    L.llsm_gpu_batch_set_pbpeffect.argtypes = [vp, C.c_int, vp, vp, vp]
    L.llsm_gpu_batch_phasesync_rps.argtypes = [vp, C.c_int]
    L.llsm_gpu_batch_phasepropagate.argtypes = [vp, C.c_int]
    L.llsm_gpu_batch_retime.argtypes = [vp, vp, P_fp, P_int]
    L.llsm_gpu_retime_uniform_positions.argtypes = [C.c_int, C.c_int, P_fp]
    L.llsm_gpu_retime_uniform_positions.restype = None
    L.llsm_gpu_batch_pitch_formant.argtypes = [vp, P_fp, P_fp, C.c_int]
    L.llsm_gpu_batch_splice.argtypes = [vp, vp, C.POINTER(SpliceMap)]
    try:                                                 # (as below: an experiment build of an earlier commit lacks the smoothing)
        L.llsm_gpu_batch_smooth.argtypes = [vp, P_int, C.c_int]
        L.llsm_gpu_join_radii.argtypes = [C.c_int, P_int, P_int, P_fp, C.c_int, P_int]
    except AttributeError:
        if "LLSM_AMD_LIB" not in os.environ:
            raise
    L.llsm_gpu_f0_default_options.argtypes = [C.POINTER(F0Options)]
    L.llsm_gpu_f0_default_options.restype = None
    L.llsm_gpu_f0_plan.argtypes = [C.POINTER(F0Options), fp, P_int, P_int, P_int, P_int]
    L.llsm_gpu_batch_estimate_f0.argtypes = [vp, C.POINTER(F0Options)]
    try:                                                 # (as above: an experiment build of an earlier commit lacks the tracker)
        L.llsm_gpu_f0_track_default_options.argtypes = [C.POINTER(F0TrackOptions)]
        L.llsm_gpu_f0_track_default_options.restype = None
        L.llsm_gpu_f0_track_check.argtypes = [C.POINTER(F0TrackOptions)]
        L.llsm_gpu_batch_track_f0.argtypes = [vp, C.POINTER(F0Options), C.POINTER(F0TrackOptions)]
    except AttributeError:
        if "LLSM_AMD_LIB" not in os.environ:
            raise
    try:                                                 # (as above: an experiment build of an earlier commit lacks the alignment)
        L.llsm_gpu_align_default_options.argtypes = [C.POINTER(AlignOptions)]
        L.llsm_gpu_align_default_options.restype = None
        L.llsm_gpu_align_check.argtypes = [C.POINTER(AlignOptions), C.c_int, C.c_int]
        L.llsm_gpu_batch_align.argtypes = [vp, vp, C.c_int, P_int, P_int, C.POINTER(AlignOptions), P_fp, P_fp]
    except AttributeError:
        if "LLSM_AMD_LIB" not in os.environ:
            raise
    try:                                                 # (as above: an experiment build of an earlier commit lacks the banded alignment)
        L.llsm_gpu_batch_align_band.argtypes = [vp, vp, C.c_int, P_int, P_int, P_int, C.POINTER(AlignOptions), P_fp, P_fp]
        L.llsm_gpu_align_band_min.argtypes = [C.c_int, C.c_int]
        L.llsm_gpu_align_band_rows.argtypes = [C.c_int, C.c_int, C.c_int, P_int, P_int]
    except AttributeError:
        if "LLSM_AMD_LIB" not in os.environ:
            raise
    try:                                                 # (as above: an experiment build of an earlier commit lacks the slope pattern)
        L.llsm_gpu_batch_align_slope.argtypes = [vp, vp, C.c_int, P_int, P_int, C.POINTER(AlignOptions), P_fp, P_fp]
        L.llsm_gpu_align_slope_rows.argtypes = [C.c_int, C.c_int, P_int, P_int]
    except AttributeError:
        if "LLSM_AMD_LIB" not in os.environ:
            raise
    try:                                                 # (as above: an experiment build of an earlier commit lacks the banded slope pattern)
        L.llsm_gpu_batch_align_band_slope.argtypes = [vp, vp, C.c_int, P_int, P_int, P_int, C.POINTER(AlignOptions), P_fp, P_fp]
        L.llsm_gpu_align_band_slope_min.argtypes = [C.c_int, C.c_int]
        L.llsm_gpu_align_band_slope_rows.argtypes = [C.c_int, C.c_int, C.c_int, P_int, P_int]
    except AttributeError:
        if "LLSM_AMD_LIB" not in os.environ:
            raise
    try:                                                 # (as above: an experiment build of an earlier commit lacks the band around a line)
        L.llsm_gpu_batch_align_around.argtypes = [vp, vp, C.c_int, P_int, P_int, P_int, P_int, C.c_int, C.POINTER(AlignOptions), P_fp, P_fp]
        L.llsm_gpu_align_around_rows.argtypes = [C.c_int, C.c_int, P_int, C.c_int, C.c_int, P_int, P_int]
        L.llsm_gpu_align_around_min.argtypes = [C.c_int, C.c_int, P_int, C.c_int]
        L.llsm_gpu_align_center_line.argtypes = [C.c_int, C.c_int, P_fp, C.c_int, C.c_int, P_int]
    except AttributeError:
        if "LLSM_AMD_LIB" not in os.environ:
            raise
    try:                                                 # (as above: an experiment build of an earlier commit lacks the pooling and the pyramid)
        L.llsm_gpu_pool_frames.argtypes = [C.c_int, C.c_int]
        L.llsm_gpu_batch_pool_code.argtypes = [vp, C.c_int, C.c_int, P_int, P_fp]
        L.llsm_gpu_batch_align_pyramid.argtypes = [vp, vp, C.c_int, P_int, P_int, C.c_int, C.c_int, C.c_int, C.POINTER(AlignOptions),
                                                   P_fp, P_fp, P_int, P_int]
    except AttributeError:
        if "LLSM_AMD_LIB" not in os.environ:
            raise
    try:                                                 # (as above: an experiment build of an earlier commit lacks the open-ended alignment)
        L.llsm_gpu_align_sub_rows.argtypes = [C.c_int, C.c_int, C.c_int, P_int, P_int]
        L.llsm_gpu_batch_align_sub.argtypes = [vp, vp, C.c_int, P_int, P_int, C.c_int, C.POINTER(AlignOptions), P_fp, P_int, P_fp, P_fp]
        L.llsm_gpu_batch_align_sub_plane.argtypes = [vp, vp, C.c_longlong]; L.llsm_gpu_batch_align_sub_plane.restype = C.c_longlong
    except AttributeError:
        if "LLSM_AMD_LIB" not in os.environ:
            raise
    try:                                                 # (as above: an experiment build of an earlier commit lacks the selection)
        L.llsm_gpu_select_default_options.argtypes = [C.POINTER(SelectOptions)]
        L.llsm_gpu_select_default_options.restype = None
        L.llsm_gpu_select_check.argtypes = [C.POINTER(SelectOptions), C.c_int, C.c_int]
        L.llsm_gpu_batch_select.argtypes = [vp, vp, C.POINTER(SelectOptions), P_int, P_fp, P_fp]
    except AttributeError:
        if "LLSM_AMD_LIB" not in os.environ:
            raise
    try:                                                 # (as above: an experiment build of an earlier commit lacks the chained selection)
        L.llsm_gpu_batch_select_chain.argtypes = [vp, vp, C.POINTER(SelectOptions), P_int, P_fp, P_fp]
    except AttributeError:
        if "LLSM_AMD_LIB" not in os.environ:
            raise
    try:                                                 # (as above: an experiment build of an earlier commit lacks the coder)
        L.llsm_gpu_batch_enable_coder.argtypes = [vp, C.c_int, C.c_int]
        L.llsm_gpu_batch_coder_dimension.argtypes = [vp]
        L.llsm_gpu_batch_encode.argtypes = [vp]
        L.llsm_gpu_batch_decode.argtypes = [vp, C.c_int]
    except AttributeError:
        if "LLSM_AMD_LIB" not in os.environ:
            raise
    try:                                                 # (as above: an experiment build of an earlier commit lacks the blob export)
        L.llsm_blob_bytes.restype = C.c_size_t
        L.llsm_blob_bytes.argtypes = [C.c_int] * 7
        L.llsm_gpu_batch_blob_sizes.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        L.llsm_gpu_batch_download_blobs.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.llsm_gpu_batch_download_blob_block.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    except AttributeError:
        if "LLSM_AMD_LIB" not in os.environ:
            raise
    L.llsm_chunk_to_flat_l1.argtypes = [C.POINTER(Chunk), C.POINTER(FlatL1), C.c_int]
    L.llsm_flat_l1_to_chunk.argtypes = [C.POINTER(FlatL1), C.c_int, C.POINTER(Chunk)]
    L.llsm_chunk_tolayer1.argtypes = [C.POINTER(Chunk), C.c_int]
    L.llsm_chunk_tolayer0.argtypes = [C.POINTER(Chunk)]
    L.llsm_frame_tolayer0.argtypes = [C.POINTER(Container), C.POINTER(Container)]
    L.llsm_conf_checklayer1.argtypes = [C.POINTER(Container)]
    L.llsm_frame_checklayer1.argtypes = [C.POINTER(Container)]
    L.llsm_create_pbpeffect.restype = vp
    L.llsm_create_pbpeffect.argtypes = [vp, vp]
    L.llsm_gpu_plan_index.argtypes = [C.c_int, C.c_int, C.c_int, fp, fp, fp, fp]
    # reference entry points
    L.llsm_create_aoptions.restype = C.POINTER(AOptions)
    L.llsm_delete_aoptions.argtypes = [C.POINTER(AOptions)]
    L.llsm_create_soptions.restype = C.POINTER(SOptions)
    L.llsm_create_soptions.argtypes = [fp]
    L.llsm_delete_soptions.argtypes = [C.POINTER(SOptions)]
    L.llsm_aoptions_toconf.restype = C.POINTER(Container)
    L.llsm_aoptions_toconf.argtypes = [C.POINTER(AOptions), fp]
    L.llsm_analyze.restype = C.POINTER(Chunk)
    L.llsm_analyze.argtypes = [C.POINTER(AOptions), P_fp, C.c_int, fp, P_fp, C.c_int, C.POINTER(P_fp)]
    L.llsm_synthesize.restype = C.POINTER(Output)
    L.llsm_synthesize.argtypes = [C.POINTER(SOptions), C.POINTER(Chunk)]
    L.llsm_delete_output.argtypes = [C.POINTER(Output)]
    L.llsm_delete_chunk.argtypes = [C.POINTER(Chunk)]
    L.llsm_copy_chunk.restype = C.POINTER(Chunk)
    L.llsm_copy_chunk.argtypes = [C.POINTER(Chunk)]
    L.llsm_create_chunk.restype = C.POINTER(Chunk)
    L.llsm_create_chunk.argtypes = [C.POINTER(Container), C.c_int]
    L.llsm_chunk_getf0.restype = P_fp
    L.llsm_chunk_getf0.argtypes = [C.POINTER(Chunk), P_int]
    L.llsm_chunk_phasesync_rps.argtypes = [C.POINTER(Chunk), C.c_int]
    L.llsm_chunk_phasepropagate.argtypes = [C.POINTER(Chunk), C.c_int]
    L.llsm_chunk_to_flat.argtypes = [C.POINTER(Chunk), C.POINTER(FlatParams), C.c_int]
    L.llsm_flat_to_chunk.argtypes = [C.POINTER(FlatParams), C.c_int, C.POINTER(Chunk)]
    L.llsm_container_get.restype = vp
    L.llsm_container_get.argtypes = [C.POINTER(Container), C.c_int]
    L.llsm_create_container.restype = C.POINTER(Container)
    L.llsm_create_container.argtypes = [C.c_int]
    L.llsm_copy_container.restype = C.POINTER(Container)
    L.llsm_copy_container.argtypes = [C.POINTER(Container)]
    L.llsm_copy_container_inplace.argtypes = [C.POINTER(Container), C.POINTER(Container)]
    L.llsm_delete_container.argtypes = [C.POINTER(Container)]
    L.llsm_container_attach_.argtypes = [C.POINTER(Container), C.c_int, vp, vp, vp]
    L.llsm_container_remove.argtypes = [C.POINTER(Container), C.c_int]
    L.llsm_create_fp.restype = P_fp
    L.llsm_create_fp.argtypes = [fp]
    L.llsm_create_int.restype = P_int
    L.llsm_create_int.argtypes = [C.c_int]
    L.llsm_create_fparray.restype = P_fp
    L.llsm_create_fparray.argtypes = [C.c_int]
    L.llsm_copy_fparray.restype = P_fp
    L.llsm_copy_fparray.argtypes = [P_fp]
    L.llsm_fparray_length.argtypes = [P_fp]
    L.llsm_delete_fparray.argtypes = [P_fp]
    L.llsm_create_hmframe.restype = C.POINTER(HMFrame)
    L.llsm_create_hmframe.argtypes = [C.c_int]
    L.llsm_copy_hmframe.restype = C.POINTER(HMFrame)
    L.llsm_copy_hmframe.argtypes = [C.POINTER(HMFrame)]
    L.llsm_delete_hmframe.argtypes = [C.POINTER(HMFrame)]
    L.llsm_hmframe_phaseshift.argtypes = [C.POINTER(HMFrame), fp]
    L.llsm_create_nmframe.restype = C.POINTER(NMFrame)
    L.llsm_create_nmframe.argtypes = [C.c_int, C.c_int, C.c_int]
    L.llsm_copy_nmframe.restype = C.POINTER(NMFrame)
    L.llsm_copy_nmframe.argtypes = [C.POINTER(NMFrame)]
    L.llsm_delete_nmframe.argtypes = [C.POINTER(NMFrame)]
    L.llsm_create_frame.restype = C.POINTER(Container)
    L.llsm_create_frame.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.llsm_frame_checklayer0.argtypes = [C.POINTER(Container)]
    L.llsm_conf_checklayer0.argtypes = [C.POINTER(Container)]
    L.llsm_create_rtsynth_buffer.restype = vp
    L.llsm_create_rtsynth_buffer.argtypes = [C.POINTER(SOptions), C.POINTER(Container), C.c_int]
    L.llsm_delete_rtsynth_buffer.argtypes = [vp]
    L.llsm_rtsynth_buffer_getlatency.argtypes = [vp]
    L.llsm_rtsynth_buffer_numoutput.argtypes = [vp]
    L.llsm_rtsynth_buffer_feed.argtypes = [vp, C.POINTER(Container)]
    L.llsm_rtsynth_buffer_fetch.argtypes = [vp, P_fp]
    L.llsm_rtsynth_buffer_fetch_decomposed.argtypes = [vp, P_fp, P_fp]
    L.llsm_rtsynth_buffer_clear.argtypes = [vp]
    L.llsm_create_rtsynth_group.restype = vp
    L.llsm_create_rtsynth_group.argtypes = [C.POINTER(SOptions), C.POINTER(Container), C.c_int, C.c_int]
    L.llsm_delete_rtsynth_group.argtypes = [vp]
    L.llsm_rtsynth_group_getlatency.argtypes = [vp]
    L.llsm_rtsynth_group_numoutput.argtypes = [vp, C.c_int]
    L.llsm_rtsynth_group_feed.argtypes = [vp, C.POINTER(C.POINTER(Container))]
    L.llsm_rtsynth_group_fetch.argtypes = [vp, C.c_int, P_fp, P_fp, C.c_int]
    L.llsm_rtsynth_group_fetch_all.argtypes = [vp, P_fp, P_fp, C.c_int, P_int]
    L.llsm_gpu_rt_graph.argtypes = [C.c_int]
    L.llsm_gpu_shared_f0_tiles.argtypes = [C.c_int]
    L.llsm_gpu_synth_tables.argtypes = [C.c_int]
    L.llsm_gpu_pbp_real_ifft.argtypes = [C.c_int]
    L.llsm_gpu_rt_fused.argtypes = [C.c_int]
    L.llsm_gpu_rt_direct.argtypes = [C.c_int]
    L.llsm_gpu_rt_pipeline.argtypes = [C.c_int]
    L.llsm_gpu_analysis_overlap.argtypes = [C.c_int]
    L.llsm_gpu_rt_graph_hops.restype = C.c_longlong
    _lib = L
    return L


class LlsmError(RuntimeError):
    pass


def _check(rc, what):
    if rc != 0:
        raise LlsmError(f"{what}: {load().llsm_gpu_last_error().decode()}")


def make_aoptions(**kw):
    """llsm_create_aoptions() defaults (layer0.c:27-43) with overrides; the
    returned object keeps its chanfreq storage alive."""
    o = AOptions()
    o.thop, o.maxnhar, o.maxnhar_e, o.npsd, o.nchannel = 0.005, 100, 4, 256, 4
    o.lip_radius, o.f0_refine, o.hm_method, o.rel_winsize = 1.5, 1, HMCZT, 4.0
    cf = kw.pop("chanfreq", [2000.0, 4000.0, 8000.0])
    for k, v in kw.items():
        setattr(o, k, v)
    o._cf = (fp * max(len(cf), 1))(*cf)
    o.chanfreq = C.cast(o._cf, P_fp)
    return o


def retime_uniform_positions(nfrm_src, nfrm_dst):
    """the source positions llsm_gpu_batch_retime uses without a map (llsm_gpu_retime_uniform_positions)"""
    pos = np.zeros(max(int(nfrm_dst), 0), np.float32)
    load().llsm_gpu_retime_uniform_positions(int(nfrm_src), int(nfrm_dst), pos.ctypes.data_as(P_fp))
    return pos


def make_f0_options(**kw):
    """llsm_gpu_f0_default_options() with overrides"""
    o = F0Options()
    load().llsm_gpu_f0_default_options(C.byref(o))
    for k, v in kw.items():
        if k not in dict(F0Options._fields_):
            raise TypeError("llsm_gpu_f0_options has no member " + k)
        setattr(o, k, v)
    return o


def make_f0_track_options(**kw):
    """llsm_gpu_f0_track_default_options() with overrides"""
    o = F0TrackOptions()
    load().llsm_gpu_f0_track_default_options(C.byref(o))
    for k, v in kw.items():
        if k not in dict(F0TrackOptions._fields_):
            raise TypeError("llsm_gpu_f0_track_options has no member " + k)
        setattr(o, k, v)
    return o


def make_align_options(**kw):
    """llsm_gpu_align_default_options() with overrides"""
    o = AlignOptions()
    load().llsm_gpu_align_default_options(C.byref(o))
    for k, v in kw.items():
        if k not in dict(AlignOptions._fields_):
            raise TypeError("llsm_gpu_align_options has no member " + k)
        setattr(o, k, v)
    return o


def align_band_min(na, nb):
    """the least connected band of an na x nb pair (llsm_gpu_align_band_min, rule B1 of llsm_gpu_batch_align_band)"""
    r = load().llsm_gpu_align_band_min(int(na), int(nb))
    if r < 0:
        raise LlsmError("align_band_min: " + load().llsm_gpu_last_error().decode())
    return int(r)


def align_band_rows(na, nb, band):
    """(lo, hi): the first and the last column of every row of an na x nb pair under this band, int32 [na] each
    (llsm_gpu_align_band_rows); a band that is negative or not connected is refused"""
    lo = np.zeros(max(int(na), 0), np.int32); hi = np.zeros(max(int(na), 0), np.int32)
    _check(load().llsm_gpu_align_band_rows(int(na), int(nb), int(band), lo.ctypes.data_as(P_int), hi.ctypes.data_as(P_int)),
           "align_band_rows")
    return lo, hi


def align_slope_rows(na, nb):
    """(lo, hi): the first and the last column of every row of an na x nb pair under the slope pattern, int32 [na] each,
    lo > hi where no path stops on the row (llsm_gpu_align_slope_rows, rule L1 of llsm_gpu_batch_align_slope); a pair that
    is not admissible is refused"""
    lo = np.zeros(max(int(na), 0), np.int32); hi = np.zeros(max(int(na), 0), np.int32)
    _check(load().llsm_gpu_align_slope_rows(int(na), int(nb), lo.ctypes.data_as(P_int), hi.ctypes.data_as(P_int)),
           "align_slope_rows")
    return lo, hi


def align_sub_rows(na, nb, slope=False):
    """(lo, hi): the column range of every row of a query of na frames inside a take of nb with free ends, int32 [na] each:
    every column, or with slope ceil(i / 2) ... nb - 1 (llsm_gpu_align_sub_rows, rule Q1 of llsm_gpu_batch_align_sub); a
    pair that is not admissible is refused"""
    lo = np.zeros(max(int(na), 0), np.int32); hi = np.zeros(max(int(na), 0), np.int32)
    _check(load().llsm_gpu_align_sub_rows(int(na), int(nb), int(slope), lo.ctypes.data_as(P_int), hi.ctypes.data_as(P_int)),
           "align_sub_rows")
    return lo, hi


def align_band_slope_min(na, nb):
    """the least band that is connected for the slope pattern on an na x nb pair (llsm_gpu_align_band_slope_min, rule K1 of
    llsm_gpu_batch_align_band_slope); a pair that is not admissible is refused"""
    r = load().llsm_gpu_align_band_slope_min(int(na), int(nb))
    if r < 0:
        raise LlsmError("align_band_slope_min: " + load().llsm_gpu_last_error().decode())
    return int(r)


def align_band_slope_rows(na, nb, band):
    """(lo, hi): the first and the last column of every row of the region of the slope pattern inside `band` columns of the
    diagonal, int32 [na] each, lo > hi (1, 0) where no path stops on the row (llsm_gpu_align_band_slope_rows, rule K1); a
    pair that is not admissible and a band that is negative or not connected for the pattern are refused"""
    lo = np.zeros(max(int(na), 0), np.int32); hi = np.zeros(max(int(na), 0), np.int32)
    _check(load().llsm_gpu_align_band_slope_rows(int(na), int(nb), int(band), lo.ctypes.data_as(P_int), hi.ctypes.data_as(P_int)),
           "align_band_slope_rows")
    return lo, hi


def align_around_rows(na, nb, center, band, slope=False):
    """(lo, hi): the first and the last column of every row of an na x nb pair within `band` columns of the centre line
    `center` (na ints), int32 [na] each: the band's rows, or with slope the rows of the region of the slope pattern, lo > hi
    (1, 0) where no path stops on the row (llsm_gpu_align_around_rows, rule A1 of llsm_gpu_batch_align_around); a line that
    is not valid, a band that is negative or not connected and, with slope, a pair that is not admissible are refused"""
    c = np.ascontiguousarray(center, np.int32)
    assert c.shape == (max(int(na), 0),), (c.shape, na)
    lo = np.zeros(len(c), np.int32); hi = np.zeros(len(c), np.int32)
    _check(load().llsm_gpu_align_around_rows(int(na), int(nb), c.ctypes.data_as(P_int), int(band), int(slope),
                                             lo.ctypes.data_as(P_int), hi.ctypes.data_as(P_int)), "align_around_rows")
    return lo, hi


def align_around_min(na, nb, center, slope=False):
    """the least band that is connected around the centre line `center` of an na x nb pair, for the plain moves or with slope
    for the slope pattern (llsm_gpu_align_around_min, rule A1)"""
    c = np.ascontiguousarray(center, np.int32)
    assert c.shape == (max(int(na), 0),), (c.shape, na)
    r = load().llsm_gpu_align_around_min(int(na), int(nb), c.ctypes.data_as(P_int), int(slope))
    if r < 0:
        raise LlsmError("align_around_min: " + load().llsm_gpu_last_error().decode())
    return int(r)


def align_center_line(pos_c, nb_c, na, nb):
    """the positions pos_c of an alignment of a coarse pair (len(pos_c) x nb_c frames) as the centre line of the fine pair
    of na x nb frames, int32 [na]: interpolated, scaled, rounded and made non-decreasing (llsm_gpu_align_center_line)"""
    pc = np.ascontiguousarray(pos_c, np.float32)
    assert pc.ndim == 1, pc.shape
    c = np.zeros(max(int(na), 0), np.int32)
    _check(load().llsm_gpu_align_center_line(len(pc), int(nb_c), pc.ctypes.data_as(P_fp), int(na), int(nb),
                                             c.ctypes.data_as(P_int)), "align_center_line")
    return c


def pool_frames(nfrm, factor):
    """the coarse frames of an utterance of nfrm frames pooled by `factor`, ceil(nfrm / factor) (llsm_gpu_pool_frames, rule P1
    of llsm_gpu_batch_pool_code); nfrm < 1 and a factor outside [1, 64] are refused"""
    r = load().llsm_gpu_pool_frames(int(nfrm), int(factor))
    if r < 0:
        raise LlsmError("pool_frames: " + load().llsm_gpu_last_error().decode())
    return int(r)


def make_select_options(**kw):
    """llsm_gpu_select_default_options() with overrides"""
    o = SelectOptions()
    load().llsm_gpu_select_default_options(C.byref(o))
    for k, v in kw.items():
        if k not in dict(SelectOptions._fields_):
            raise TypeError("llsm_gpu_select_options has no member " + k)
        setattr(o, k, v)
    return o


def f0_plan(fs, **kw):
    """the sizes the F0 options imply at fs, as a dict lmin, lmax, W, nfft (llsm_gpu_f0_plan); LlsmError where
    llsm_gpu_batch_estimate_f0 would refuse them"""
    o = make_f0_options(**kw)
    v = [C.c_int() for _ in range(4)]
    _check(load().llsm_gpu_f0_plan(C.byref(o), fs, *[C.byref(x) for x in v]), "f0_plan")
    return dict(zip(("lmin", "lmax", "W", "nfft"), (x.value for x in v)))


WARP_PSD = 1                                               # LLSM_GPU_WARP_PSD (llsm_gpu_batch_pitch_formant)


def per_frame_ratio(value, nfrm):
    """a pitch_formant ratio as total_frames float32 values: None stays None (1 everywhere), a scalar is every frame's,
    n_utt values are one per utterance, total_frames values one per frame (the two agree when every utterance has one
    frame)"""
    if value is None:
        return None
    nfrm = np.asarray(nfrm, np.int64)
    F = int(nfrm.sum())
    v = np.asarray(value, np.float32)
    if v.ndim == 0:
        return np.full(F, v, np.float32)
    if v.shape == (F,):
        return np.ascontiguousarray(v)
    if v.shape == (len(nfrm),):
        return np.repeat(v, nfrm).astype(np.float32)
    raise ValueError("ratio of shape %s: expected a scalar, %d utterance values or %d frame values"
                     % (v.shape, len(nfrm), F))


# LLSM_GPU_SMOOTH_* (llsm_gpu_batch_smooth)
SMOOTH_F0, SMOOTH_RD, SMOOTH_VTMAGN, SMOOTH_PSD, SMOOTH_EDC, SMOOTH_ALL = 1, 2, 4, 8, 16, 31
SMOOTH_MAX_RADIUS = 32


def per_frame_radius(value, total_frames):
    """a smooth radius as total_frames int32 values: a scalar is every frame's, total_frames values are taken as they
    are; any other shape is a ValueError"""
    F = int(total_frames)
    v = np.asarray(value)
    if v.dtype.kind not in "iu" and not np.array_equal(v, np.floor(v)):
        raise ValueError("radius holds values that are not integers")
    if v.ndim == 0:
        return np.full(F, int(v), np.int32)
    if v.shape == (F,):
        return np.ascontiguousarray(v, np.int32)
    raise ValueError("radius of shape %s: expected a scalar or %d frame values" % (v.shape, F))


def join_radii(nfrm, pos_a, utt_a=None, reach=8):
    """(radius, n_joins): the int32 radii Batch.smooth takes, from the lists Batch.splice renders
    (llsm_gpu_join_radii): reach on the two frames at every join, falling by one per frame to 0; nfrm: the frame counts
    of the destination's utterances, pos_a and utt_a (None: every frame's own utterance) one entry per frame"""
    n = np.ascontiguousarray(nfrm, np.int32)
    F = int(n.astype(np.int64).sum()) if (n >= 0).all() else 0
    p = np.ascontiguousarray(pos_a, np.float32)
    u = None if utt_a is None else np.ascontiguousarray(utt_a, np.int32)
    if (n >= 0).all() and (p.shape != (F,) or (u is not None and u.shape != (F,))):
        raise ValueError("pos_a / utt_a: expected %d frame values" % F)
    radius = np.zeros(F, np.int32)
    k = load().llsm_gpu_join_radii(len(n), n.ctypes.data_as(P_int), None if u is None else u.ctypes.data_as(P_int),
                                   p.ctypes.data_as(P_fp), int(reach), radius.ctypes.data_as(P_int))
    if k < 0:
        raise LlsmError("join_radii: " + load().llsm_gpu_last_error().decode())
    return radius, int(k)


def make_soptions(fs, **kw):
    o = SOptions()
    o.fs, o.use_iczt, o.use_l1, o.iczt_param_a, o.iczt_param_b = fs, 1, 0, 0.275, 2.26
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class Context:
    def __init__(self, device=0, stream=None):
        self.L = load()
        self.h = self.L.llsm_gpu_create_context(device, stream)
        if not self.h:
            raise LlsmError("llsm_gpu_create_context: " + self.L.llsm_gpu_last_error().decode())

    def close(self):
        if self.h:
            self.L.llsm_gpu_delete_context(self.h)
            self.h = None

    def sync(self):
        _check(self.L.llsm_gpu_synchronize(self.h), "synchronize")

    def set_profiling(self, on, only=None):
        """per-kernel HIP events on / off; only: the events around ONE kernel name (the least instrument in a timed region)"""
        if only is not None:
            self.L.llsm_gpu_profile_only(self.h, only.encode())
            self.L.llsm_gpu_set_profiling(self.h, 2 if on else 0)
        else:
            self.L.llsm_gpu_set_profiling(self.h, int(bool(on)))

    def reset_profile(self):
        self.L.llsm_gpu_reset_profile(self.h)

    def fft_selftest(self, z, inverse=False):
        """run the wavefront FFT on rows of z (complex64 [count, 2^logn]); diagnostic"""
        import numpy as np
        z = np.ascontiguousarray(z, np.complex64)
        count, n = z.shape
        out = np.empty_like(z)
        _check(self.L.llsm_gpu_fft_selftest(self.h, int(n).bit_length() - 1, count, int(inverse),
                                            z.ctypes.data, out.ctypes.data), "fft_selftest")
        return out

    def profile(self):
        cap = 64
        names = (C.c_char_p * cap)(); ms = (C.c_double * cap)(); n = (C.c_int * cap)()
        k = self.L.llsm_gpu_get_profile(self.h, cap, names, ms, n)
        return {names[i].decode(): (ms[i], n[i]) for i in range(min(k, cap))}


class Batch:
    """Device-resident batch of utterances (llsm_gpu.h)."""

    def __init__(self, ctx, aopt, fs, nx, nfrm):
        self.ctx, self.L, self.aopt, self.fs = ctx, ctx.L, aopt, fs
        nx = np.ascontiguousarray(nx, np.int32); nfrm = np.ascontiguousarray(nfrm, np.int32)
        self.h = self.L.llsm_gpu_create_batch(ctx.h, C.byref(aopt), fs, len(nx),
                                              nx.ctypes.data_as(P_int), nfrm.ctypes.data_as(P_int))
        if not self.h:
            raise LlsmError("llsm_gpu_create_batch: " + self.L.llsm_gpu_last_error().decode())
        self.layout = Layout()
        self.L.llsm_gpu_batch_layout(self.h, C.byref(self.layout))
        n = len(nx) + 1
        self.x_off = np.zeros(n, np.int32); self.frm_off = np.zeros(n, np.int32); self.y_off = np.zeros(n, np.int32)
        self.L.llsm_gpu_batch_offsets(self.h, self.x_off.ctypes.data_as(P_int),
                                      self.frm_off.ctypes.data_as(P_int), self.y_off.ctypes.data_as(P_int))

    def close(self):
        if self.h:
            self.L.llsm_gpu_delete_batch(self.h)
            self.h = None

    def shape(self, aid):
        l = self.layout
        F, me = l.total_frames, max(l.maxnhar_e, 1)
        ns = getattr(self, "nspec", 0)
        return {A_RD: (F,), A_VTMAGN: (F, ns), A_VSPHSE: (F, l.maxnhar), A_NVSPHSE: (F,), A_PBPSYN: (F,), A_HAS_HM: (F,),
                A_CODE: (F, self.coder_dimension),
                A_X: (l.total_samples,), A_XRES: (l.total_samples,), A_F0: (F,), A_NHAR: (F,),
                A_NHAR_E: (F,), A_HAS_PSDRES: (F,), A_AMPL: (F, l.maxnhar), A_PHSE: (F, l.maxnhar),
                A_PSD: (F, l.npsd), A_PSDRES: (F, l.npsd), A_EDC: (F, l.nchannel),
                A_EENV_AMPL: (F, l.nchannel, me), A_EENV_PHSE: (F, l.nchannel, me),
                A_Y: (l.total_out,), A_YSIN: (l.total_out,), A_YNOISE: (l.total_out,),
                A_WHITE: (l.n_utt, l.nchannel, l.ntemplate_ext)}[aid]

    def upload(self, aid, a):
        dt = np.int32 if aid in _INT_ARRAYS else np.float32
        a = np.ascontiguousarray(a, dt)
        assert a.shape == self.shape(aid), (a.shape, self.shape(aid))
        _check(self.L.llsm_gpu_batch_upload(self.h, aid, a.ctypes.data, a.nbytes), "upload")

    def download(self, aid, out=None):
        """copy array `aid` to the host; `out` (e.g. from pinned_array) is filled in place"""
        dt = np.int32 if aid in _INT_ARRAYS else np.float32
        a = np.zeros(self.shape(aid), dt) if out is None else out
        assert a.dtype == dt and a.nbytes == int(np.prod(self.shape(aid))) * 4
        _check(self.L.llsm_gpu_batch_download(self.h, aid, a.ctypes.data, a.nbytes), "download")
        return a

    def pinned_array(self, aid):
        """page-locked numpy array shaped like array `aid` (llsm_gpu_alloc_host); the caller keeps
        the returned object alive and releases it with free_pinned"""
        dt = np.int32 if aid in _INT_ARRAYS else np.float32
        shape = self.shape(aid)
        n = int(np.prod(shape)) * 4
        self.L.llsm_gpu_alloc_host.restype = C.c_void_p
        self.L.llsm_gpu_alloc_host.argtypes = [C.c_size_t]
        p = self.L.llsm_gpu_alloc_host(n)
        if not p:
            raise LlsmError("llsm_gpu_alloc_host")
        buf = (C.c_ubyte * max(n, 1)).from_address(p)
        a = np.frombuffer(buf, dtype=dt, count=n // 4).reshape(shape)
        self.__dict__.setdefault("_pinned", {})[id(a)] = p
        return a

    def free_pinned(self, a):
        self.L.llsm_gpu_free_host.argtypes = [C.c_void_p]
        self.L.llsm_gpu_free_host(C.c_void_p(self._pinned.pop(id(a))))

    def device_ptr(self, aid):
        return self.L.llsm_gpu_batch_device_ptr(self.h, aid)

    def analyze(self):
        _check(self.L.llsm_gpu_batch_analyze(self.h), "analyze")

    # ---- layer 1 (llsm_gpu.h)
    L1_IDS = (A_RD, A_VTMAGN, A_VSPHSE, A_NVSPHSE, A_PBPSYN, A_HAS_HM)

    def enable_layer1(self, nfft):
        _check(self.L.llsm_gpu_batch_enable_layer1(self.h, nfft), "enable_layer1")
        self.nspec = nfft // 2 + 1

    def tolayer1(self, nfft):
        _check(self.L.llsm_gpu_batch_tolayer1(self.h, nfft), "tolayer1")
        self.nspec = nfft // 2 + 1

    def tolayer0(self, only_missing=False):
        _check(self.L.llsm_gpu_batch_tolayer0(self.h, int(only_missing)), "tolayer0")

    # ---- edits (llsm_gpu.h): the middle of the time-stretch recipe on the device
    def phasesync_rps(self, layer1_based=False):
        _check(self.L.llsm_gpu_batch_phasesync_rps(self.h, int(layer1_based)), "phasesync_rps")

    def phasepropagate(self, sign):
        _check(self.L.llsm_gpu_batch_phasepropagate(self.h, int(sign)), "phasepropagate")

    def retime(self, src, pos=None, psdres_src=None):
        """this batch's rows <- the frames of batch `src` blended onto this batch's frame grid (llsm_gpu_batch_retime);
        pos: total_frames float32 source positions (None: the uniform map), psdres_src: total_frames source frame
        indices for the PSDRES rows (None: floor(pos))"""
        p = r = None
        if pos is not None:
            p = np.ascontiguousarray(pos, np.float32)
            assert p.shape == (self.layout.total_frames,), p.shape
        if psdres_src is not None:
            r = np.ascontiguousarray(psdres_src, np.int32)
            assert r.shape == (self.layout.total_frames,), r.shape
        _check(self.L.llsm_gpu_batch_retime(self.h, src.h, None if p is None else p.ctypes.data_as(P_fp),
                                            None if r is None else r.ctypes.data_as(P_int)), "retime")
        self.nspec = src.nspec

    def splice(self, src, pos_a, utt_a=None, utt_b=None, pos_b=None, mix=None):
        """this batch's rows <- frames gathered from any utterances of batch `src` and blended between two sides
        (llsm_gpu_batch_splice); every argument is None or total_frames values in this batch's frame order: pos_a / pos_b
        float32 positions in frames of utterance utt_a / utt_b (utt_a None: the output frame's own utterance), mix the
        weight of side b; utt_b, pos_b and mix go together"""
        F = self.layout.total_frames

        def arr(v, dt):
            if v is None:
                return None
            v = np.ascontiguousarray(v, dt)
            assert v.shape == (F,), v.shape
            return v
        keep = [arr(utt_a, np.int32), arr(pos_a, np.float32), arr(utt_b, np.int32), arr(pos_b, np.float32),
                arr(mix, np.float32)]
        m = SpliceMap(*[None if v is None else v.ctypes.data_as(P_int if v.dtype == np.int32 else P_fp) for v in keep])
        _check(self.L.llsm_gpu_batch_splice(self.h, src.h, C.byref(m)), "splice")
        self.nspec = src.nspec

    def pitch_formant(self, f0_ratio=None, formant_ratio=None, warp_psd=False):
        """F0 and formant ratios on a layer-1 batch (llsm_gpu_batch_pitch_formant); each ratio is None (1), a scalar,
        n_utt values (one per utterance) or total_frames values; warp_psd: the formant warp moves the PSD row too"""
        nfrm = np.diff(self.frm_off)
        r, a = per_frame_ratio(f0_ratio, nfrm), per_frame_ratio(formant_ratio, nfrm)
        _check(self.L.llsm_gpu_batch_pitch_formant(self.h, None if r is None else r.ctypes.data_as(P_fp),
                                                   None if a is None else a.ctypes.data_as(P_fp),
                                                   WARP_PSD if warp_psd else 0), "pitch_formant")

    def smooth(self, radius, flags=SMOOTH_ALL):
        """triangular means of F0, RD, VTMAGN, PSD and EDC (flags: an OR of SMOOTH_*) along the frames, in place, from a
        snapshot of the rows (llsm_gpu_batch_smooth); radius: a scalar or total_frames ints (join_radii), 0: untouched"""
        r = per_frame_radius(radius, self.layout.total_frames)
        _check(self.L.llsm_gpu_batch_smooth(self.h, r.ctypes.data_as(P_int), int(flags)), "smooth")

    # ---- F0 estimation (llsm_gpu.h): LLSM_GPU_X -> LLSM_GPU_F0 on the device
    def estimate_f0(self, **options):
        """the F0 row from the uploaded waveforms (llsm_gpu_batch_estimate_f0); options: the members of
        llsm_gpu_f0_options, defaults where not given"""
        o = make_f0_options(**options)
        _check(self.L.llsm_gpu_batch_estimate_f0(self.h, C.byref(o)), "estimate_f0")

    def track_f0(self, f0=None, **track_options):
        """the F0 row from the uploaded waveforms through the path search (llsm_gpu_batch_track_f0); f0: a dict of
        members of llsm_gpu_f0_options or None; track_options: members of llsm_gpu_f0_track_options; defaults where
        not given"""
        o = make_f0_options(**(f0 or {}))
        t = make_f0_track_options(**track_options)
        _check(self.L.llsm_gpu_batch_track_f0(self.h, C.byref(o), C.byref(t)), "track_f0")

    def debug_plane(self, which):
        """intermediate plane `which` as a flat float32 array (llsm_gpu_batch_debug_plane; 4: the CMNDF rows of the
        last estimate_f0 / track_f0 with keep_cmndf=1, total_frames x (lmax + 1); 5: the candidate rows of the last
        track_f0, total_frames x 24; 6: the distance planes of the last align with this batch as a, pair after pair,
        each na x nb; 7 and 8: the candidate rows, total_frames x 16, and the join costs, total_frames x 64, of the last select
        with this batch as the target; 9: the band planes of the last align_band with this batch as a, pair after pair,
        each na x (2 band + 1), +inf outside the rows' ranges; 10 and 11: the state rows, total_frames x 32 (c of slots
        0 ... 15, then their bank frames; absent slots 1e30 and -1), and the join costs, total_frames x 256 (entry 16 a + j),
        of the last select_chain with this batch as the target; 12: the distance planes of the last align_slope with this
        batch as a, pair after pair, each na x nb; 13: the band planes of the last align_band_slope with this batch as a,
        laid out as plane 9; 14: the band planes of the last align_around with this batch as a, laid out as plane 9 around
        that call's centre lines; 15: the noise excitation of the last synthesize, total_out samples laid out as
        A_YNOISE, what that call's noise filter read)"""
        n = self.L.llsm_gpu_batch_debug_plane(self.h, int(which), None, 0)
        if n < 0:
            raise LlsmError("debug_plane: " + self.L.llsm_gpu_last_error().decode())
        a = np.zeros(n, np.float32)
        if self.L.llsm_gpu_batch_debug_plane(self.h, int(which), a.ctypes.data, n) != n:
            raise LlsmError("debug_plane: " + self.L.llsm_gpu_last_error().decode())
        return a

    # ---- frame coder (llsm_gpu.h): rows <-> LLSM_GPU_CODE, [total_frames][coder_dimension] float32
    def enable_coder(self, order_spec, order_bap):
        _check(self.L.llsm_gpu_batch_enable_coder(self.h, int(order_spec), int(order_bap)), "enable_coder")

    @property
    def coder_dimension(self):
        return int(self.L.llsm_gpu_batch_coder_dimension(self.h))

    def encode(self):
        _check(self.L.llsm_gpu_batch_encode(self.h), "encode")

    def decode(self, use_layer1):
        _check(self.L.llsm_gpu_batch_decode(self.h, int(use_layer1)), "decode")

    # ---- alignment (llsm_gpu.h): LLSM_GPU_CODE of two batches -> positions for splice and path costs
    def _align(self, call, name, other, utt_a, utt_b, band, options, before=(), after=()):
        """the five alignment calls: `call` of the library under `name`, with one band per pair unless band is None;
        before and after: the arguments next to the band"""
        o = make_align_options(**options)
        ua = np.ascontiguousarray(utt_a, np.int32); ub = np.ascontiguousarray(utt_b, np.int32)
        assert ua.ndim == 1 and ua.shape == ub.shape, (ua.shape, ub.shape)
        bands = () if band is None else (np.ascontiguousarray(np.broadcast_to(np.asarray(band, np.int32), ua.shape)),)
        nfrm = np.diff(self.frm_off)
        inside = (ua >= 0) & (ua < len(nfrm))                       # (an index outside is the library's to refuse)
        na = np.zeros(len(ua), np.int64); na[inside] = nfrm[ua[inside]]
        pos = np.zeros(int(na.sum()), np.float32); cost = np.zeros(len(ua), np.float32)
        _check(call(self.h, other.h, len(ua), ua.ctypes.data_as(P_int), ub.ctypes.data_as(P_int),
                    *before, *(bd.ctypes.data_as(P_int) for bd in bands), *after, C.byref(o), pos.ctypes.data_as(P_fp),
                    cost.ctypes.data_as(P_fp)), name)
        return np.split(pos, np.cumsum(na)[:-1]) if len(ua) else [], cost

    def align(self, other, utt_a, utt_b, **options):
        """one minimum-cost monotonic path per pair (utterance utt_a[p] of this batch, utterance utt_b[p] of batch
        `other`) through the distances of their coder vectors (llsm_gpu_batch_align); options: the members of
        llsm_gpu_align_options, defaults where not given.  Returns (a list with one float32 array per pair: for every
        frame of the utterance of this batch its position in frames of the other utterance, as splice takes it; the
        float32 array of the path costs)"""
        return self._align(self.L.llsm_gpu_batch_align, "align", other, utt_a, utt_b, None, options)

    def align_band(self, other, utt_a, utt_b, band, **options):
        """align within `band` columns of the straight diagonal (llsm_gpu_batch_align_band): what long utterances need,
        whose full matrices align refuses.  band: an int, or one int per pair.  Returns what align returns"""
        return self._align(self.L.llsm_gpu_batch_align_band, "align_band", other, utt_a, utt_b, band, options)

    def align_slope(self, other, utt_a, utt_b, **options):
        """align with the local slope of the path held within [1/2, 2] (llsm_gpu_batch_align_slope): no frame of either
        utterance is held for more than two frames of the other, none is skipped.  Pairs outside nb - 1 <= 2 (na - 1),
        na - 1 <= 2 (nb - 1) are refused.  Returns what align returns"""
        return self._align(self.L.llsm_gpu_batch_align_slope, "align_slope", other, utt_a, utt_b, None, options)

    def align_band_slope(self, other, utt_a, utt_b, band, **options):
        """align_slope within `band` columns of the straight diagonal (llsm_gpu_batch_align_band_slope): slopes within
        [1/2, 2] for utterances whose full matrices align_slope refuses.  band: an int, or one int per pair; a pair that
        align_slope refuses and a band below align_band_slope_min of the pair are refused.  Returns what align_band returns"""
        return self._align(self.L.llsm_gpu_batch_align_band_slope, "align_band_slope", other, utt_a, utt_b, band, options)

    def align_around(self, other, utt_a, utt_b, center, band, slope=False, **options):
        """align within `band` columns of a centre line per pair (llsm_gpu_batch_align_around): the fine pass of a
        coarse-to-fine alignment, whose lines align_center_line makes from the positions of the coarse pass.  center: a
        list with one int array per pair (as many columns as the utterance of this batch has frames), or all of them as one
        flat array; band: an int, or one int per pair; slope: the moves of align_band_slope instead of those of align_band.
        Returns what align_band returns"""
        flat = isinstance(center, np.ndarray) and center.ndim == 1
        c = np.ascontiguousarray(center if flat else np.concatenate([np.asarray(x).reshape(-1) for x in center] or [np.zeros(0)]), np.int32)
        ua = np.asarray(utt_a).reshape(-1)
        nfrm = np.diff(self.frm_off)
        need = int(sum(nfrm[u] for u in ua if 0 <= u < len(nfrm)))  # (an index outside is the library's to refuse)
        if len(c) != need:
            raise ValueError("align_around: center has %d columns, the pairs have %d frames" % (len(c), need))
        return self._align(self.L.llsm_gpu_batch_align_around, "align_around", other, utt_a, utt_b, band, options,
                           before=(c.ctypes.data_as(P_int),), after=(int(slope),))

    def _frames_of(self, utts):
        """the frames of the listed utterances, 0 for an index outside (which is the library's to refuse)"""
        u = np.ascontiguousarray(utts, np.int32).reshape(-1)
        nfrm = np.diff(self.frm_off)
        inside = (u >= 0) & (u < len(nfrm))
        n = np.zeros(len(u), np.int64); n[inside] = nfrm[u[inside]]
        return u, n

    def pool_code(self, utts, factor):
        """the coder vectors of the listed utterances (repeats allowed, any order) pooled by `factor`: the mean of every
        `factor` consecutive rows of A_CODE, computed on the device (llsm_gpu_batch_pool_code, rule P1) -- the input of a
        coarse alignment.  Returns a list with one float32 array [pool_frames(nfrm, factor)][coder_dimension] per entry"""
        u, n = self._frames_of(utts)
        f = int(factor)
        nc = (n + f - 1) // f if 1 <= f <= 64 else np.zeros(len(u), np.int64)      # (a factor outside is the library's to refuse)
        dim = self.coder_dimension
        dst = np.zeros((int(nc.sum()), max(dim, 0)), np.float32)
        _check(self.L.llsm_gpu_batch_pool_code(self.h, f, len(u), u.ctypes.data_as(P_int), dst.ctypes.data_as(P_fp)), "pool_code")
        return np.split(dst, np.cumsum(nc)[:-1]) if len(u) else []

    def align_pyramid(self, other, utt_a, utt_b, factor, margin, slope=False, **options):
        """coarse-to-fine alignment in one call (llsm_gpu_batch_align_pyramid): both utterances of a pair pooled by `factor`
        on the device, the pooled pair aligned (align, or align_slope with slope), its positions turned into a centre line
        (align_center_line), and the fine pair searched within max(margin * factor, align_around_min) columns of it
        (align_around).  Returns (pos, cost, center, band): what align_around returns, a list with the line of every pair
        (int32) and the int32 array of the bands that were used"""
        o = make_align_options(**options)
        ua, na = self._frames_of(utt_a)
        ub = np.ascontiguousarray(utt_b, np.int32).reshape(-1)
        assert ua.shape == ub.shape, (ua.shape, ub.shape)
        pos = np.zeros(int(na.sum()), np.float32); cost = np.zeros(len(ua), np.float32)
        center = np.zeros(int(na.sum()), np.int32); band = np.zeros(len(ua), np.int32)
        _check(self.L.llsm_gpu_batch_align_pyramid(self.h, other.h, len(ua), ua.ctypes.data_as(P_int), ub.ctypes.data_as(P_int),
                                                   int(factor), int(margin), int(slope), C.byref(o), pos.ctypes.data_as(P_fp),
                                                   cost.ctypes.data_as(P_fp), center.ctypes.data_as(P_int), band.ctypes.data_as(P_int)),
               "align_pyramid")
        cut = np.cumsum(na)[:-1]
        return (np.split(pos, cut) if len(ua) else []), cost, (np.split(center, cut) if len(ua) else []), band

    def align_sub(self, other, utt_a, utt_b, slope=False, last_row=False, **options):
        """open-ended alignment (llsm_gpu_batch_align_sub): the whole of utterance utt_a[p] of this batch, the query, against
        some stretch of utterance utt_b[p] of `other`, the take; the path starts and ends anywhere along the take.  slope:
        the moves of align_slope instead of those of align.  Returns (pos, span, cost): pos as align returns it, span int32
        [n_pairs][2], the first and the last frame of the take on each path, and the float32 array of the path costs; with
        last_row also a list with acc of the query's last row along the take, one float32 array [nb] per pair"""
        o = make_align_options(**options)
        ua, na = self._frames_of(utt_a)
        ub, nb = other._frames_of(utt_b)
        assert ua.shape == ub.shape, (ua.shape, ub.shape)
        pos = np.zeros(int(na.sum()), np.float32); cost = np.zeros(len(ua), np.float32)
        span = np.zeros((len(ua), 2), np.int32)
        rows = np.zeros(int(nb.sum()) if last_row else 0, np.float32)
        _check(self.L.llsm_gpu_batch_align_sub(self.h, other.h, len(ua), ua.ctypes.data_as(P_int), ub.ctypes.data_as(P_int),
                                               int(slope), C.byref(o), pos.ctypes.data_as(P_fp), span.ctypes.data_as(P_int),
                                               cost.ctypes.data_as(P_fp), rows.ctypes.data_as(P_fp) if last_row else None),
               "align_sub")
        self._sub_shapes = [(int(n), int(m)) for n, m in zip(na, nb)]  # (of the planes the call has just rewritten)
        out = (np.split(pos, np.cumsum(na)[:-1]) if len(ua) else []), span, cost
        return out + ((np.split(rows, np.cumsum(nb)[:-1]) if len(ua) else []),) if last_row else out

    def align_sub_planes(self):
        """the distance planes of the last successful align_sub with this batch as the query side
        (llsm_gpu_batch_align_sub_plane), cut per pair: a list with one float32 array [na][nb] per pair of that call"""
        n = self.L.llsm_gpu_batch_align_sub_plane(self.h, None, 0)
        if n < 0:
            raise LlsmError("align_sub_planes: " + self.L.llsm_gpu_last_error().decode())
        a = np.zeros(n, np.float32)
        if self.L.llsm_gpu_batch_align_sub_plane(self.h, a.ctypes.data, n) != n:
            raise LlsmError("align_sub_planes: " + self.L.llsm_gpu_last_error().decode())
        shapes = getattr(self, "_sub_shapes", [])
        assert n == sum(r * c for r, c in shapes), (n, shapes)
        cut = np.cumsum([r * c for r, c in shapes])[:-1]
        return [x.reshape(sh) for x, sh in zip(np.split(a, cut), shapes)]

    # ---- unit selection (llsm_gpu.h): LLSM_GPU_CODE of this batch and of a bank -> the index lists splice renders
    def select(self, bank, opt=None, **options):
        """for every frame of this batch the frame of `bank` that renders it (llsm_gpu_batch_select): the eight nearest
        bank frames per frame, then a minimum-cost path per utterance with a join cost.  opt: a SelectOptions (None: the
        defaults), or its members as keywords.  Returns (utt int32 [total_frames], pos float32 [total_frames], as splice
        takes them for utt_a / pos_a with src = bank; cost float32 [n_utt])"""
        assert opt is None or not options
        o = opt if opt is not None else make_select_options(**options)
        n = int(self.frm_off[-1])
        utt = np.zeros(n, np.int32); pos = np.zeros(n, np.float32); cost = np.zeros(self.layout.n_utt, np.float32)
        _check(self.L.llsm_gpu_batch_select(self.h, bank.h, C.byref(o), utt.ctypes.data_as(P_int), pos.ctypes.data_as(P_fp),
                                            cost.ctypes.data_as(P_fp)), "select")
        return utt, pos, cost

    def select_chain(self, bank, opt=None, **options):
        """select with the continuations of the previous frame's states added to every frame's candidates
        (llsm_gpu_batch_select_chain): where the bank holds similar renditions the path stays in one recording instead of
        paying joins.  Arguments and results as select; planes 10 and 11 of debug_plane instead of 7 and 8"""
        assert opt is None or not options
        o = opt if opt is not None else make_select_options(**options)
        n = int(self.frm_off[-1])
        utt = np.zeros(n, np.int32); pos = np.zeros(n, np.float32); cost = np.zeros(self.layout.n_utt, np.float32)
        _check(self.L.llsm_gpu_batch_select_chain(self.h, bank.h, C.byref(o), utt.ctypes.data_as(P_int),
                                                  pos.ctypes.data_as(P_fp), cost.ctypes.data_as(P_fp)), "select_chain")
        return utt, pos, cost

    # ---- export as chunk blobs (llsm_gpu.h): the wire format of csrc/wire.cpp, packed on the device
    def _blob_range(self, utt0, n):
        return int(utt0), int(self.layout.n_utt - utt0 if n is None else n)

    def blob_sizes(self, utt0=0, n=None):
        """bytes of the blobs of utterances [utt0, utt0 + n) as the batch stands now (llsm_gpu_batch_blob_sizes)"""
        utt0, n = self._blob_range(utt0, n)
        sizes = (C.c_size_t * max(n, 1))()
        _check(self.L.llsm_gpu_batch_blob_sizes(self.h, utt0, n, sizes), "blob_sizes")
        return [int(sizes[k]) for k in range(n)]

    def download_blobs(self, utt0=0, n=None, as_bytes=False):
        """the blobs of utterances [utt0, utt0 + n): a list of uint8 arrays (8-byte aligned: llsm_blob_view takes them), or
        of bytes objects (llsm_gpu_batch_download_blobs)"""
        utt0, n = self._blob_range(utt0, n)
        sizes = self.blob_sizes(utt0, n)
        words = [np.zeros((s + 7) // 8, np.uint64) for s in sizes]
        ptrs = (C.c_void_p * max(n, 1))(*[w.ctypes.data for w in words])
        caps = (C.c_size_t * max(n, 1))(*sizes)
        _check(self.L.llsm_gpu_batch_download_blobs(self.h, utt0, n, ptrs, caps), "download_blobs")
        out = [w.view(np.uint8)[:s] for w, s in zip(words, sizes)]
        return [o.tobytes() for o in out] if as_bytes else out

    def download_blob_block(self, block, utt0=0, n=None):
        """the same blobs back to back in `block` (a uint8 array, page-locked or not): returns the n + 1 offsets
        (llsm_gpu_batch_download_blob_block)"""
        utt0, n = self._blob_range(utt0, n)
        assert block.dtype == np.uint8 and block.flags.c_contiguous
        offs = (C.c_size_t * (max(n, 0) + 1))()
        _check(self.L.llsm_gpu_batch_download_blob_block(self.h, utt0, n, C.c_void_p(block.ctypes.data), block.nbytes, offs),
               "download_blob_block")
        return [int(o) for o in offs]

    def synthesize(self, sopt, seed=0, injected_white=False):
        _check(self.L.llsm_gpu_batch_synthesize(self.h, C.byref(sopt), seed, int(injected_white)), "synthesize")

    PARAM_IDS = (A_F0, A_NHAR, A_AMPL, A_PHSE, A_PSD, A_PSDRES, A_HAS_PSDRES, A_EDC, A_NHAR_E,
                 A_EENV_AMPL, A_EENV_PHSE)

    def pinned_params_block(self):
        """the eleven parameter rows as ONE page-locked block laid out like the device's (llsm_gpu_batch_params_layout):
        returns (block as uint8 array, {array id: view}); moved in one copy by transfer_params_block; release the block
        with free_pinned"""
        total = C.c_size_t(0); offs = (C.c_size_t * 11)(); ids = (C.c_int * 11)()
        self.L.llsm_gpu_batch_params_layout.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        _check(self.L.llsm_gpu_batch_params_layout(self.h, C.byref(total), offs, ids), "params_layout")
        self.L.llsm_gpu_alloc_host.restype = C.c_void_p
        self.L.llsm_gpu_alloc_host.argtypes = [C.c_size_t]
        p = self.L.llsm_gpu_alloc_host(total.value)
        if not p:
            raise LlsmError("llsm_gpu_alloc_host")
        raw = np.frombuffer((C.c_ubyte * max(total.value, 1)).from_address(p), dtype=np.uint8)
        self.__dict__.setdefault("_pinned", {})[id(raw)] = p
        views = {}
        for k in range(11):
            aid = int(ids[k]); shape = self.shape(aid); n = int(np.prod(shape))
            dt = np.int32 if aid in _INT_ARRAYS else np.float32
            views[aid] = raw[offs[k]:offs[k] + 4 * n].view(dt).reshape(shape)
        return raw, views

    def transfer_params_block(self, raw, to_device=False):
        self.L.llsm_gpu_batch_transfer_params.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _check(self.L.llsm_gpu_batch_transfer_params(self.h, int(to_device), C.c_void_p(raw.ctypes.data)), "transfer_params")

    def transfer_many(self, arrays, to_device=False):
        """{array id: host array}: every copy enqueued, the stream waited for once (llsm_gpu_batch_transfer_many)"""
        n = len(arrays)
        ids = (C.c_int * n)(*arrays.keys())
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrays.values()])
        nb = (C.c_size_t * n)(*[a.nbytes for a in arrays.values()])
        self.L.llsm_gpu_batch_transfer_many.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        _check(self.L.llsm_gpu_batch_transfer_many(self.h, int(to_device), n, ids, ptrs, nb), "transfer_many")

    def download_params(self):
        return {aid: self.download(aid) for aid in self.PARAM_IDS}

    def upload_params(self, params):
        for aid, a in params.items():
            self.upload(aid, a)
