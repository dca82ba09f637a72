"""ctypes binding of libbnflac.so -- the Python mirror of LibFLACSharp.

``LibFLAC`` mirrors ``Library/LibFLACSharp/LibFLACSharp.cs`` (class LibFLAC, :18): the same
decoder entry points (:42-85, :175-185), enums (:24-36, :89-173, :248-280) and callback
delegate shapes (:187-212), bound to the MI355X library instead of the Win32 LibFlac.dll.
``BatchDecoder`` wraps the device-pointer API (include/bnflac.h part 2).

The library is GPU-only: loading works anywhere (symbol checks run on CPU-only hosts);
decoding without a usable GPU fails loudly.
"""
from __future__ import annotations

import ctypes
import enum
from typing import Optional

import numpy as np

from ._lib import lib_path


class StreamDecoderState(enum.IntEnum):  # LibFLACSharp.cs:24-36
    SearchForMetadata = 0
    ReadMetadata = 1
    SearchForFrameSync = 2
    ReadFrame = 3
    EndOfStream = 4
    OggError = 5
    SeekError = 6
    Aborted = 7
    MemoryAllocationError = 8
    Uninitialized = 9


class StreamDecoderReadStatus(enum.IntEnum):  # :89-110
    ReadStatusContinue = 0
    ReadStatusEndOfStream = 1
    ReadStatusAbort = 2


class StreamDecoderSeekStatus(enum.IntEnum):  # :113-127
    SeekStatusOk = 0
    SeekStatusError = 1
    SeekStatusUnsupported = 2


class StreamDecoderTellStatus(enum.IntEnum):  # :130-144
    TellStatusOK = 0
    TellStatusError = 1
    TellStatusUnsupported = 2


class StreamDecoderLengthStatus(enum.IntEnum):  # :147-161
    LengthStatusOk = 0
    LengthStatusError = 1
    LengthStatusUnsupported = 2


class StreamDecoderWriteStatus(enum.IntEnum):  # :163-173
    WriteStatusContinue = 0
    WriteStatusAbort = 1


class DecodeError(enum.IntEnum):  # :262-268
    LostSync = 0
    BadHeader = 1
    FrameCrcMismatch = 2
    UnparsableStream = 3


class FLACMetaDataType(enum.IntEnum):  # :270-280
    StreamInfo = 0
    Padding = 1
    Application = 2
    Seekable = 3
    VorbisComment = 4
    CueSheet = 5
    Picture = 6
    Undefined = 7


class FrameHeader(ctypes.Structure):  # :224-234 (offsets 0/4/8/12/16/20/24/32)
    _fields_ = [("BlockSize", ctypes.c_int32), ("SampleRate", ctypes.c_int32), ("Channels", ctypes.c_int32),
                ("ChannelAssignment", ctypes.c_int32), ("BitsPerSample", ctypes.c_int32),
                ("NumberType", ctypes.c_int32), ("FrameOrSampleNumber", ctypes.c_int64), ("Crc", ctypes.c_uint8)]


class FLACMetaData(ctypes.Structure):  # :282-293 (Data[] marshalled from offset 12)
    _pack_ = 4
    _fields_ = [("MetaDataType", ctypes.c_int32), ("IsLast", ctypes.c_int32), ("Length", ctypes.c_int32),
                ("Data", ctypes.c_uint8 * 100)]


class FLACStreamInfo(ctypes.Structure):  # :295-319 explicit layout over FLACMetaData.Data
    _pack_ = 1
    _fields_ = [("_hdr", ctypes.c_int32), ("MinBlocksize", ctypes.c_int32), ("MaxBlocksize", ctypes.c_int32),
                ("min_framesize", ctypes.c_int32), ("max_framesize", ctypes.c_int32), ("SampleRate", ctypes.c_int32),
                ("Channels", ctypes.c_int32), ("BitsPerSample", ctypes.c_int32), ("TotalSamplesHi", ctypes.c_int32),
                ("TotalSamplesLo", ctypes.c_int32)]


_DEC = ctypes.c_void_p
DecoderReadCallback = ctypes.CFUNCTYPE(ctypes.c_int, _DEC, ctypes.POINTER(ctypes.c_uint8),
                                       ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p)
DecoderSeekCallback = ctypes.CFUNCTYPE(ctypes.c_int, _DEC, ctypes.c_uint64, ctypes.c_void_p)
DecoderTellCallback = ctypes.CFUNCTYPE(ctypes.c_int, _DEC, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p)
DecoderLengthCallback = ctypes.CFUNCTYPE(ctypes.c_int, _DEC, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p)
DecoderEofCallback = ctypes.CFUNCTYPE(ctypes.c_int, _DEC, ctypes.c_void_p)
DecoderWriteCallbackWithStatus = ctypes.CFUNCTYPE(ctypes.c_int, _DEC, ctypes.c_void_p,
                                                  ctypes.POINTER(ctypes.POINTER(ctypes.c_int32)), ctypes.c_void_p)
Decoder_WriteCallback = DecoderWriteCallbackWithStatus  # declared void in C# (:205-206); see init_file
Decoder_MetadataCallback = ctypes.CFUNCTYPE(None, _DEC, ctypes.c_void_p, ctypes.c_void_p)
Decoder_ErrorCallback = ctypes.CFUNCTYPE(None, _DEC, ctypes.c_int, ctypes.c_void_p)

DECODER_SYMBOLS = [
    "FLAC__stream_decoder_new", "FLAC__stream_decoder_finish", "FLAC__stream_decoder_delete",
    "FLAC__stream_decoder_init_file", "FLAC__stream_decoder_process_single",
    "FLAC__stream_decoder_process_until_end_of_metadata", "FLAC__stream_decoder_process_until_end_of_stream",
    "FLAC__stream_decoder_seek_absolute", "FLAC__stream_decoder_get_decode_position",
    "FLAC__stream_decoder_get_total_samples", "FLAC__stream_decoder_get_channels",
    "FLAC__stream_decoder_get_bits_per_sample", "FLAC__stream_decoder_get_sample_rate",
    "FLAC__stream_decoder_get_state", "FLAC__stream_decoder_reset", "FLAC__stream_decoder_init_stream",
    "FLAC__stream_decoder_set_md5_checking", "FLAC__stream_decoder_get_md5_checking",
]
BATCH_SYMBOLS = ["bnflac_ctx_create", "bnflac_ctx_destroy", "bnflac_last_error", "bnflac_device_count",
                 "bnflac_index_frames", "bnflac_decode_frames", "bnflac_parse_frames", "bnflac_decode_parsed",
                 "bnflac_out_stride", "bnflac_debug_set_ablate", "bnflac_debug_stats", "bnflac_debug_set_parse_wave", "bnflac_debug_parse_wave_stats",
                 "bnflac_debug_set_decode_sys", "bnflac_debug_decode_seg_launches", "bnflac_debug_last_route",
                 "bnflac_md5_interleaved32", "bnflac_index_stream",
                 "bnflac_index_streams", "bnflac_md5_layout", "bnflac_md5_streams",
                 "bnflac_scan_streams", "bnflac_scan_stream_host",
                 "bnflac_select_ranges", "bnflac_select_ranges_host", "bnflac_gather_ranges",
                 "bnflac_select_windows", "bnflac_select_windows_host",
                 "bnflac_select_windows_shared", "bnflac_select_windows_shared_host",
                 "bnflac_window_health", "bnflac_window_health_host",
                 "bnflac_index_streams_resync", "bnflac_resync_plan_host", "bnflac_debug_index_candidates",
                 "bnflac_gather_ranges_f32", "bnflac_gather_ranges_f32_host",
                 "bnflac_gather_ranges_f32_rs", "bnflac_gather_ranges_f32_rs_host",
                 "bnflac_resample_design", "bnflac_resample_request",
                 "bnflac_gather_ranges_mel", "bnflac_gather_ranges_mel_host", "bnflac_mel_design", "bnflac_mel_request",
                 "bnflac_debug_set_crc_mode", "bnflac_debug_crc_handoff"]
READER_SYMBOLS = ["bnflac_reader_open", "bnflac_reader_params", "bnflac_reader_read", "bnflac_reader_close",
                  "bnflac_reader_last_error", "bnflac_reader_seek", "bnflac_reader_read_filereader",
                  "bnflac_reader_pool_release"]

_LIB = None


def load() -> ctypes.CDLL:
    """Load libbnflac.so and declare signatures (no GPU work)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    L = ctypes.CDLL(lib_path("libbnflac.so"))
    b, u, i, p = ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_void_p
    L.FLAC__stream_decoder_new.restype = p
    for n in ("finish", "delete", "process_single", "process_until_end_of_metadata",
              "process_until_end_of_stream", "reset"):
        f = getattr(L, "FLAC__stream_decoder_" + n)
        f.restype, f.argtypes = b, [p]
    L.FLAC__stream_decoder_init_file.restype = i
    L.FLAC__stream_decoder_init_file.argtypes = [p, ctypes.c_char_p, Decoder_WriteCallback,
                                                 Decoder_MetadataCallback, Decoder_ErrorCallback, p]
    L.FLAC__stream_decoder_init_stream.restype = i
    L.FLAC__stream_decoder_init_stream.argtypes = [p, DecoderReadCallback, DecoderSeekCallback, DecoderTellCallback,
                                                   DecoderLengthCallback, DecoderEofCallback,
                                                   DecoderWriteCallbackWithStatus, Decoder_MetadataCallback,
                                                   Decoder_ErrorCallback, p]
    L.FLAC__stream_decoder_seek_absolute.restype, L.FLAC__stream_decoder_seek_absolute.argtypes = b, [p, ctypes.c_uint64]
    L.FLAC__stream_decoder_get_decode_position.restype = b
    L.FLAC__stream_decoder_get_decode_position.argtypes = [p, ctypes.POINTER(ctypes.c_uint64)]
    L.FLAC__stream_decoder_get_total_samples.restype = ctypes.c_uint64
    L.FLAC__stream_decoder_get_total_samples.argtypes = [p]
    for n in ("get_channels", "get_bits_per_sample", "get_sample_rate", "get_state"):
        f = getattr(L, "FLAC__stream_decoder_" + n)
        f.restype, f.argtypes = u, [p]
    L.bnflac_last_error.restype = ctypes.c_char_p
    L.bnflac_ctx_create.restype, L.bnflac_ctx_create.argtypes = i, [i, ctypes.POINTER(p)]
    L.bnflac_ctx_destroy.argtypes = [p]
    L.bnflac_index_frames.restype = i
    L.bnflac_index_frames.argtypes = [p, p, ctypes.c_uint64, p, ctypes.c_uint32, p, p]
    L.bnflac_decode_frames.restype = i
    L.bnflac_decode_frames.argtypes = [p, p, ctypes.c_uint64, p, ctypes.c_uint32, p, p, ctypes.c_uint64, i, p,
                                       ctypes.c_uint64, p, p]
    L.bnflac_parse_frames.restype = i
    L.bnflac_parse_frames.argtypes = [p, p, ctypes.c_uint64, p, ctypes.c_uint32, p, p, ctypes.c_uint64, p, p]
    L.bnflac_decode_parsed.restype = i
    L.bnflac_decode_parsed.argtypes = [p, p, ctypes.c_uint64, ctypes.c_uint32, p, i, p, ctypes.c_uint64, p, p]
    L.bnflac_debug_set_ablate.argtypes = [ctypes.c_uint32]
    L.bnflac_debug_set_parse_wave.argtypes = [ctypes.c_int]
    L.bnflac_debug_set_decode_sys.argtypes = [ctypes.c_int]
    L.bnflac_debug_set_crc_mode.argtypes = [ctypes.c_int]
    L.bnflac_debug_crc_handoff.restype = i
    L.bnflac_debug_crc_handoff.argtypes = [p, p, ctypes.c_uint32]
    L.bnflac_debug_decode_seg_launches.restype, L.bnflac_debug_decode_seg_launches.argtypes = ctypes.c_uint64, []
    L.bnflac_debug_last_route.restype, L.bnflac_debug_last_route.argtypes = None, [ctypes.POINTER(ctypes.c_uint32)]
    L.bnflac_debug_parse_wave_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    L.bnflac_debug_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    L.bnflac_debug_stats.restype = ctypes.c_int
    L.bnflac_out_stride.restype = ctypes.c_uint32
    L.bnflac_out_stride.argtypes = [i, p]
    L.FLAC__stream_decoder_set_md5_checking.restype = b
    L.FLAC__stream_decoder_set_md5_checking.argtypes = [p, b]
    L.FLAC__stream_decoder_get_md5_checking.restype = b
    L.FLAC__stream_decoder_get_md5_checking.argtypes = [p]
    L.bnflac_index_stream.restype = i
    L.bnflac_index_stream.argtypes = [p, p, ctypes.c_uint64, ctypes.c_uint64, p, p, p, p, ctypes.c_uint32, p, p]
    L.bnflac_index_streams.restype = i
    L.bnflac_index_streams.argtypes = [p, p, ctypes.c_uint64, p, ctypes.c_uint32, p, ctypes.c_uint32, p, p, p,
                                       ctypes.c_uint32, p, p, p, p]
    L.bnflac_index_streams_resync.restype = i
    L.bnflac_index_streams_resync.argtypes = [p, p, ctypes.c_uint64, p, ctypes.c_uint32, p, ctypes.c_uint32, p, p, p,
                                              ctypes.c_uint32, p, p, p, p, p]
    L.bnflac_resync_plan_host.restype = i
    L.bnflac_resync_plan_host.argtypes = [p, ctypes.c_uint32, p, ctypes.c_uint32, ctypes.c_uint32, p, ctypes.c_uint32, p, p,
                                          p, p]
    L.bnflac_debug_index_candidates.restype = i
    L.bnflac_debug_index_candidates.argtypes = [p, p, ctypes.c_uint32, p]
    L.bnflac_reader_open.restype = i
    L.bnflac_reader_open.argtypes = [i, p, ctypes.c_uint64, i, ctypes.c_uint32, ctypes.POINTER(p)]
    L.bnflac_reader_params.restype = i
    L.bnflac_reader_params.argtypes = [p, p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
    L.bnflac_reader_read.restype = ctypes.c_int64
    L.bnflac_reader_read.argtypes = [p, p, ctypes.c_uint64]
    L.bnflac_reader_close.argtypes = [p]
    L.bnflac_reader_pool_release.argtypes = [ctypes.c_int]
    L.bnflac_reader_pool_release.restype = ctypes.c_int
    L.bnflac_reader_read_filereader.restype = ctypes.c_int64
    L.bnflac_reader_read_filereader.argtypes = [p, p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    L.bnflac_reader_seek.restype = i
    L.bnflac_reader_seek.argtypes = [p, ctypes.c_uint64]
    L.bnflac_reader_last_error.restype = ctypes.c_char_p
    L.bnflac_md5_interleaved32.restype = i
    L.bnflac_md5_interleaved32.argtypes = [p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, p]
    L.bnflac_md5_layout.restype, L.bnflac_md5_layout.argtypes = ctypes.c_uint32, [i, p]
    L.bnflac_md5_streams.restype = i
    L.bnflac_md5_streams.argtypes = [p, p, ctypes.c_uint64, i, p, p, ctypes.c_uint32, p, p, p, p, p]
    L.bnflac_scan_streams.restype = i
    L.bnflac_scan_streams.argtypes = [p, p, ctypes.c_uint64, p, ctypes.c_uint32, p, p, p, p, p]
    L.bnflac_scan_stream_host.restype = i
    L.bnflac_scan_stream_host.argtypes = [p, ctypes.c_uint64, p, p]
    L.bnflac_select_ranges.restype = i
    L.bnflac_select_ranges.argtypes = [p, p, p, ctypes.c_uint32, p, p, ctypes.c_uint32, p, p, p, ctypes.c_uint32, p, p, p,
                                       p, p]
    L.bnflac_select_ranges_host.restype = i
    L.bnflac_select_ranges_host.argtypes = [p, ctypes.c_uint32, p, p, ctypes.c_uint32, p, p, ctypes.c_uint32, p, p, p, p]
    L.bnflac_select_windows.restype = i
    L.bnflac_select_windows.argtypes = [p, p, p, ctypes.c_uint32, p, p, ctypes.c_uint32, p, ctypes.c_uint32, p, p,
                                        ctypes.c_uint32, p, p, p, p, p]
    L.bnflac_select_windows_host.restype = i
    L.bnflac_select_windows_host.argtypes = [p, ctypes.c_uint32, p, p, ctypes.c_uint32, p, ctypes.c_uint32, p,
                                             ctypes.c_uint32, p, p, p, p]
    L.bnflac_select_windows_shared.restype = i
    L.bnflac_select_windows_shared.argtypes = [p, p, p, ctypes.c_uint32, p, p, ctypes.c_uint32, p, ctypes.c_uint32, p, p,
                                               ctypes.c_uint32, p, p, p, p, p]
    L.bnflac_select_windows_shared_host.restype = i
    L.bnflac_select_windows_shared_host.argtypes = [p, ctypes.c_uint32, p, p, ctypes.c_uint32, p, ctypes.c_uint32, p,
                                                    ctypes.c_uint32, p, p, p, p]
    L.bnflac_window_health.restype = i
    L.bnflac_window_health.argtypes = [p, p, ctypes.c_uint32, p, p, ctypes.c_uint32, p, p, p, ctypes.c_uint32, p, p, p]
    L.bnflac_window_health_host.restype = i
    L.bnflac_window_health_host.argtypes = [p, ctypes.c_uint32, p, p, ctypes.c_uint32, p, p, p, ctypes.c_uint32, p, p]
    L.bnflac_gather_ranges.restype = i
    L.bnflac_gather_ranges.argtypes = [p, p, ctypes.c_uint64, i, p, p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64,
                                       p, p, p]
    L.bnflac_gather_ranges_f32.restype = i
    L.bnflac_gather_ranges_f32.argtypes = [p, p, ctypes.c_uint64, i, p, p, ctypes.c_uint32, ctypes.c_uint32,
                                           ctypes.c_uint64, ctypes.c_uint32, p, p, p]
    L.bnflac_gather_ranges_f32_host.restype = i
    L.bnflac_gather_ranges_f32_host.argtypes = [p, ctypes.c_uint64, i, p, p, ctypes.c_uint32, ctypes.c_uint32,
                                                ctypes.c_uint64, ctypes.c_uint32, p, p]
    L.bnflac_gather_ranges_f32_rs.restype = i
    L.bnflac_gather_ranges_f32_rs.argtypes = [p, p, ctypes.c_uint64, i, p, p, ctypes.c_uint32, p, p, ctypes.c_uint32,
                                              ctypes.c_uint64, ctypes.c_uint32, p, p, p]
    L.bnflac_gather_ranges_f32_rs_host.restype = i
    L.bnflac_gather_ranges_f32_rs_host.argtypes = [p, ctypes.c_uint64, i, p, p, ctypes.c_uint32, p, p, ctypes.c_uint32,
                                                   ctypes.c_uint64, ctypes.c_uint32, p, p]
    L.bnflac_resample_design.restype = ctypes.c_int64
    L.bnflac_resample_design.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double, ctypes.c_double,
                                         ctypes.c_double, p, p, ctypes.c_uint64]
    L.bnflac_resample_request.restype = i
    L.bnflac_resample_request.argtypes = [p, ctypes.c_uint64, ctypes.c_uint64, p, p, p]
    L.bnflac_gather_ranges_mel.restype = i
    L.bnflac_gather_ranges_mel.argtypes = [p, p, ctypes.c_uint64, i, p, p, ctypes.c_uint32, p, p, p, ctypes.c_uint32,
                                           ctypes.c_uint64, ctypes.c_uint32, p, p, p]
    L.bnflac_gather_ranges_mel_host.restype = i
    L.bnflac_gather_ranges_mel_host.argtypes = [p, ctypes.c_uint64, i, p, p, ctypes.c_uint32, p, p, p, ctypes.c_uint32,
                                                ctypes.c_uint64, ctypes.c_uint32, p, p]
    L.bnflac_mel_design.restype = ctypes.c_int64
    L.bnflac_mel_design.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double,
                                    ctypes.c_double, p, p, ctypes.c_uint64, p, ctypes.c_uint64]
    L.bnflac_mel_request.restype = i
    L.bnflac_mel_request.argtypes = [p, ctypes.c_uint64, ctypes.c_uint64, p, p, p]
    _LIB = L
    return L


class LibFLAC:
    """Static-style facade named like the C# class (LibFLACSharp.cs:18)."""

    @staticmethod
    def _l():
        return load()

    @staticmethod
    def FLAC__stream_decoder_new():
        return LibFLAC._l().FLAC__stream_decoder_new()

    @staticmethod
    def FLAC__stream_decoder_finish(ctx):
        return bool(LibFLAC._l().FLAC__stream_decoder_finish(ctx))

    @staticmethod
    def FLAC__stream_decoder_delete(ctx):
        return bool(LibFLAC._l().FLAC__stream_decoder_delete(ctx))

    @staticmethod
    def FLAC__stream_decoder_init_file(ctx, filename, write, metadata, error, user):
        fn = filename.encode() if isinstance(filename, str) else filename
        return LibFLAC._l().FLAC__stream_decoder_init_file(ctx, fn, write, metadata, error, user)

    @staticmethod
    def FLAC__stream_decoder_init_stream(ctx, read, seek, tell, length, eof, write, metadata, error, user):
        return LibFLAC._l().FLAC__stream_decoder_init_stream(ctx, read, seek, tell, length, eof, write, metadata,
                                                             error, user)

    @staticmethod
    def FLAC__stream_decoder_process_single(ctx):
        return bool(LibFLAC._l().FLAC__stream_decoder_process_single(ctx))

    @staticmethod
    def FLAC__stream_decoder_process_until_end_of_metadata(ctx):
        return bool(LibFLAC._l().FLAC__stream_decoder_process_until_end_of_metadata(ctx))

    @staticmethod
    def FLAC__stream_decoder_process_until_end_of_stream(ctx):
        return bool(LibFLAC._l().FLAC__stream_decoder_process_until_end_of_stream(ctx))

    @staticmethod
    def FLAC__stream_decoder_seek_absolute(ctx, sample):
        return bool(LibFLAC._l().FLAC__stream_decoder_seek_absolute(ctx, sample))

    @staticmethod
    def FLAC__stream_decoder_get_total_samples(ctx):
        return int(LibFLAC._l().FLAC__stream_decoder_get_total_samples(ctx))

    @staticmethod
    def FLAC__stream_decoder_get_state(ctx):
        return StreamDecoderState(LibFLAC._l().FLAC__stream_decoder_get_state(ctx))

    @staticmethod
    def FLAC__stream_decoder_get_channels(ctx):
        return int(LibFLAC._l().FLAC__stream_decoder_get_channels(ctx))

    @staticmethod
    def FLAC__stream_decoder_get_bits_per_sample(ctx):
        return int(LibFLAC._l().FLAC__stream_decoder_get_bits_per_sample(ctx))

    @staticmethod
    def FLAC__stream_decoder_get_sample_rate(ctx):
        return int(LibFLAC._l().FLAC__stream_decoder_get_sample_rate(ctx))

    @staticmethod
    def FLAC__stream_decoder_reset(ctx):
        return int(LibFLAC._l().FLAC__stream_decoder_reset(ctx))

    @staticmethod
    def FLAC__stream_decoder_set_md5_checking(ctx, value):
        return bool(LibFLAC._l().FLAC__stream_decoder_set_md5_checking(ctx, 1 if value else 0))

    @staticmethod
    def FLAC__stream_decoder_get_md5_checking(ctx):
        return bool(LibFLAC._l().FLAC__stream_decoder_get_md5_checking(ctx))


# ------------------------------------------------------------------ batch API
OUT_PLANAR32, OUT_INTERLEAVED32, OUT_FLACDECODER, OUT_FILEREADER = 0, 1, 2, 3
FRAME_INFO_BYTES = 128
ST_OK, ST_ERROR, ST_TRUNC, ST_SKIPPED = 0, 1, 2, 3

FRAME_INFO_DTYPE = np.dtype([
    ("status", "<u4"), ("err", "<i4"), ("frame_off", "<u8"), ("resume_bit", "<u8"), ("cached", "<i4"),
    ("blocksize", "<u4"), ("sample_rate", "<u4"), ("channels", "<u4"), ("assignment", "<u4"), ("bps", "<u4"),
    ("number_type", "<u4"), ("unparseable", "<u4"), ("number", "<u8"), ("out_sample", "<u8"), ("crc8", "<u4"),
    ("crc16_calc", "<u4"), ("crc16_read", "<u4"), ("crc_ok", "<u4"), ("sub_start", "<u4", (8,)), ("flags", "<u4"),
    ("reserved", "<u4")])
assert FRAME_INFO_DTYPE.itemsize == FRAME_INFO_BYTES


class StreamParams(ctypes.Structure):
    _fields_ = [("has_stream_info", ctypes.c_int32), ("min_blocksize", ctypes.c_uint32),
                ("max_blocksize", ctypes.c_uint32), ("sample_rate", ctypes.c_uint32), ("channels", ctypes.c_uint32),
                ("bps", ctypes.c_uint32), ("total_samples", ctypes.c_uint64)]

    @classmethod
    def from_synth(cls, p, total_samples=0):
        bs = p.blocksize
        mn = p.bs_min if p.variable_blocksize else bs
        mx = p.bs_max if p.variable_blocksize else bs
        return cls(1, mn, mx, p.sample_rate, p.channels, p.bps, total_samples)


class StreamDesc(ctypes.Structure):
    """bnflac_stream_desc: one stream of an index_streams batch."""
    _fields_ = [("begin", ctypes.c_uint64), ("end", ctypes.c_uint64), ("first_offset", ctypes.c_uint64),
                ("total_samples", ctypes.c_uint64)]


STREAM_DESC_DTYPE = np.dtype([("begin", "<u8"), ("end", "<u8"), ("first_offset", "<u8"), ("total_samples", "<u8")])
assert STREAM_DESC_DTYPE.itemsize == ctypes.sizeof(StreamDesc)


SCAN_OK, SCAN_NO_MARKER, SCAN_TRUNCATED, SCAN_NO_STREAMINFO, SCAN_TOO_MANY_BLOCKS, SCAN_BAD_RANGE = range(6)
SCAN_MAX_BLOCKS = 1024
# StreamMeta.flags
META_ID3, META_DIFFERS, META_MD5_ZERO, META_SEEKTABLE = 1, 2, 4, 8


class StreamMeta(ctypes.Structure):
    """bnflac_stream_meta: one stream's record of scan_streams / scan_stream_host."""
    _fields_ = [("status", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("nblocks", ctypes.c_uint32),
                ("id3_bytes", ctypes.c_uint32), ("sp", StreamParams), ("min_framesize", ctypes.c_uint32),
                ("max_framesize", ctypes.c_uint32), ("first_offset", ctypes.c_uint64)]


STREAM_META_BYTES = 64
STREAM_META_DTYPE = np.dtype([
    ("status", "<u4"), ("flags", "<u4"), ("nblocks", "<u4"), ("id3_bytes", "<u4"), ("has_stream_info", "<i4"),
    ("min_blocksize", "<u4"), ("max_blocksize", "<u4"), ("sample_rate", "<u4"), ("channels", "<u4"), ("bps", "<u4"),
    ("total_samples", "<u8"), ("min_framesize", "<u4"), ("max_framesize", "<u4"), ("first_offset", "<u8")])
assert STREAM_META_DTYPE.itemsize == ctypes.sizeof(StreamMeta) == STREAM_META_BYTES


def scan_stream_host(data):
    """The metadata walk of scan_streams over one stream in host memory (bnflac_scan_stream_host,
    no GPU) -> (StreamMeta, the 16 md5sum bytes; zeros unless the record's status is SCAN_OK)."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    meta = StreamMeta()
    md5 = (ctypes.c_uint8 * 16)()
    rc = load().bnflac_scan_stream_host(a.ctypes.data if a.size else None, a.size, ctypes.byref(meta), md5)
    if rc != 0:
        raise RuntimeError(load().bnflac_last_error().decode())
    return meta, bytes(md5)


def meta_array(raw: np.ndarray) -> np.ndarray:
    """View a uint8 buffer of scan_streams records as a structured array."""
    return np.frombuffer(np.ascontiguousarray(raw).tobytes(), dtype=STREAM_META_DTYPE)


class SampleRange(ctypes.Structure):
    """bnflac_sample_range: one stream's window of select_ranges, in the stream's own samples."""
    _fields_ = [("first_sample", ctypes.c_uint64), ("nsamples", ctypes.c_uint64)]


class Window(ctypes.Structure):
    """bnflac_window: one stream's record of select_ranges, what gather_ranges reads."""
    _fields_ = [("pcm_first", ctypes.c_uint64), ("nsamples", ctypes.c_uint64), ("skip", ctypes.c_uint32),
                ("first_frame", ctypes.c_uint32), ("nframes", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class WindowRequest(ctypes.Structure):
    """bnflac_window_request: one crop of select_windows, a window of the stream it names."""
    _fields_ = [("stream", ctypes.c_uint64), ("first_sample", ctypes.c_uint64), ("nsamples", ctypes.c_uint64)]


SAMPLE_RANGE_DTYPE = np.dtype([("first_sample", "<u8"), ("nsamples", "<u8")])
WINDOW_REQUEST_DTYPE = np.dtype([("stream", "<u8"), ("first_sample", "<u8"), ("nsamples", "<u8")])
WINDOW_BYTES = 32
WINDOW_DTYPE = np.dtype([("pcm_first", "<u8"), ("nsamples", "<u8"), ("skip", "<u4"), ("first_frame", "<u4"),
                         ("nframes", "<u4"), ("flags", "<u4")])
assert SAMPLE_RANGE_DTYPE.itemsize == ctypes.sizeof(SampleRange) == 16
assert WINDOW_DTYPE.itemsize == ctypes.sizeof(Window) == WINDOW_BYTES
assert WINDOW_REQUEST_DTYPE.itemsize == ctypes.sizeof(WindowRequest) == 24
WIN_CLIPPED, WIN_EMPTY, WIN_NO_STREAM = 1, 2, 4           # Window.flags (WIN_NO_STREAM: select_windows only)
SEL_OVERFLOW, SEL_BAD_TABLES, SEL_NO_STREAM = 1, 2, 4     # select_ranges / select_windows status word 0
TO_THE_END = (1 << 64) - 1             # SampleRange.nsamples: up to the stream's end


def window_array(raw: np.ndarray) -> np.ndarray:
    """View a uint8 buffer of select_ranges window records as a structured array."""
    return np.frombuffer(np.ascontiguousarray(raw).tobytes(), dtype=WINDOW_DTYPE)


def sample_ranges(ranges) -> np.ndarray:
    """[(first_sample, nsamples)] -> the table of select_ranges (SAMPLE_RANGE_DTYPE)."""
    table = np.zeros(len(ranges), dtype=SAMPLE_RANGE_DTYPE)
    for k, (first, n) in enumerate(ranges):
        if not (0 <= first <= TO_THE_END and 0 <= n <= TO_THE_END):
            raise ValueError(f"stream {k}: a window is two unsigned 64-bit numbers")
        table[k] = (first, n)
    return table


def select_ranges_host(info: np.ndarray, cap: int, stream_frames, stream_samples, ranges, sel_cap: int):
    """select_ranges over host tables (bnflac_select_ranges_host, no GPU).  info: FRAME_INFO_DTYPE
    records (at least cap of them); ranges: [(first_sample, nsamples)] or a SAMPLE_RANGE_DTYPE array.
    -> (sel_info[sel_cap], sel_frames uint32[n+1], sel_samples uint64[n+1], windows[n], status uint32[4])"""
    info = np.ascontiguousarray(info, dtype=FRAME_INFO_DTYPE)
    sf = np.ascontiguousarray(stream_frames, dtype=np.uint32)
    ss = np.ascontiguousarray(stream_samples, dtype=np.uint64)
    n = len(sf) - 1
    if n < 0 or len(ss) != n + 1 or len(info) < min(cap, int(sf.max(initial=0))):
        raise ValueError("stream_frames and stream_samples hold nstreams + 1 entries, info the records below cap")
    r = ranges if isinstance(ranges, np.ndarray) and ranges.dtype == SAMPLE_RANGE_DTYPE else sample_ranges(ranges)
    r = np.ascontiguousarray(r)
    if len(r) != n:
        raise ValueError("one window per stream")
    sel = np.zeros(sel_cap, dtype=FRAME_INFO_DTYPE)
    sel_f, sel_s = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint64)
    win, status = np.zeros(n, dtype=WINDOW_DTYPE), np.zeros(4, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
    rc = load().bnflac_select_ranges_host(vp(info), cap, vp(sf), vp(ss), n, vp(r), vp(sel), sel_cap, vp(sel_f), vp(sel_s),
                                          vp(win), vp(status))
    if rc != 0:
        raise RuntimeError(load().bnflac_last_error().decode())
    return sel, sel_f, sel_s, win, status


def window_requests(reqs) -> np.ndarray:
    """[(stream, first_sample[, nsamples])] -> the table of select_windows (WINDOW_REQUEST_DTYPE);
    nsamples defaults to TO_THE_END."""
    table = np.zeros(len(reqs), dtype=WINDOW_REQUEST_DTYPE)
    for k, r in enumerate(reqs):
        r = tuple(r) if len(r) == 3 else (r[0], r[1], TO_THE_END)
        if not all(0 <= x <= TO_THE_END for x in r):
            raise ValueError(f"window {k}: a request is three unsigned 64-bit numbers")
        table[k] = r
    return table


def select_windows_host(info: np.ndarray, cap: int, stream_frames, stream_samples, requests, sel_cap: int):
    """select_windows over host tables (bnflac_select_windows_host, no GPU).  info: FRAME_INFO_DTYPE
    records (at least the ones below cap that a request's stream holds); requests:
    [(stream, first_sample[, nsamples])] or a WINDOW_REQUEST_DTYPE array, any number per stream.
    -> (sel_info[sel_cap], sel_frames uint32[k+1], sel_samples uint64[k+1], windows[k], status uint32[4])
    for k requests, in their order."""
    info = np.ascontiguousarray(info, dtype=FRAME_INFO_DTYPE)
    sf = np.ascontiguousarray(stream_frames, dtype=np.uint32)
    ss = np.ascontiguousarray(stream_samples, dtype=np.uint64)
    n = len(sf) - 1
    if n < 0 or len(ss) != n + 1 or len(info) < min(cap, int(sf.max(initial=0))):
        raise ValueError("stream_frames and stream_samples hold nstreams + 1 entries, info the records below cap")
    r = requests if isinstance(requests, np.ndarray) and requests.dtype == WINDOW_REQUEST_DTYPE else window_requests(requests)
    r = np.ascontiguousarray(r)
    k = len(r)
    sel = np.zeros(sel_cap, dtype=FRAME_INFO_DTYPE)
    sel_f, sel_s = np.zeros(k + 1, np.uint32), np.zeros(k + 1, np.uint64)
    win, status = np.zeros(k, dtype=WINDOW_DTYPE), np.zeros(4, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
    rc = load().bnflac_select_windows_host(vp(info), cap, vp(sf), vp(ss), n, vp(r), k, vp(sel), sel_cap, vp(sel_f),
                                           vp(sel_s), vp(win), vp(status))
    if rc != 0:
        raise RuntimeError(load().bnflac_last_error().decode())
    return sel, sel_f, sel_s, win, status


def select_windows_shared_host(info: np.ndarray, cap: int, stream_frames, stream_samples, requests, sel_cap: int):
    """select_windows_shared over host tables (bnflac_select_windows_shared_host, no GPU): the
    requests of select_windows_host, every frame they need selected once.
    -> (sel_info[sel_cap], windows[k], win_sel_first uint32[k], totals uint64[2] = (frames, samples),
        status uint32[4]) for k requests, the windows in their order."""
    info = np.ascontiguousarray(info, dtype=FRAME_INFO_DTYPE)
    sf = np.ascontiguousarray(stream_frames, dtype=np.uint32)
    ss = np.ascontiguousarray(stream_samples, dtype=np.uint64)
    n = len(sf) - 1
    if n < 0 or len(ss) != n + 1 or len(info) < min(cap, int(sf.max(initial=0))):
        raise ValueError("stream_frames and stream_samples hold nstreams + 1 entries, info the records below cap")
    r = requests if isinstance(requests, np.ndarray) and requests.dtype == WINDOW_REQUEST_DTYPE else window_requests(requests)
    r = np.ascontiguousarray(r)
    k = len(r)
    sel = np.zeros(sel_cap, dtype=FRAME_INFO_DTYPE)
    win, first = np.zeros(k, dtype=WINDOW_DTYPE), np.zeros(k, np.uint32)
    totals, status = np.zeros(2, np.uint64), np.zeros(4, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
    rc = load().bnflac_select_windows_shared_host(vp(info), cap, vp(sf), vp(ss), n, vp(r), k, vp(sel), sel_cap, vp(win),
                                                  vp(first), vp(totals), vp(status))
    if rc != 0:
        raise RuntimeError(load().bnflac_last_error().decode())
    return sel, win, first, totals, status


class WindowHealth(ctypes.Structure):
    """bnflac_window_health_rec: one window's record of window_health."""
    _fields_ = [("flags", ctypes.c_uint32), ("bad_frames", ctypes.c_uint32), ("crc_frames", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("bad_samples", ctypes.c_uint64), ("missing", ctypes.c_uint64)]


WINDOW_HEALTH_BYTES = 32
WINDOW_HEALTH_DTYPE = np.dtype([("flags", "<u4"), ("bad_frames", "<u4"), ("crc_frames", "<u4"), ("reserved", "<u4"),
                                ("bad_samples", "<u8"), ("missing", "<u8")])
assert WINDOW_HEALTH_DTYPE.itemsize == ctypes.sizeof(WindowHealth) == WINDOW_HEALTH_BYTES
# WindowHealth.flags; the first three are also the bits of window_health's status word 0
HEALTH_DAMAGED, HEALTH_SHORT, HEALTH_UNKNOWN, HEALTH_EMPTY, HEALTH_NO_STREAM = 1, 2, 4, 8, 16


def health_array(raw: np.ndarray) -> np.ndarray:
    """View a uint8 buffer of window_health records as a structured array."""
    return np.frombuffer(np.ascontiguousarray(raw).tobytes(), dtype=WINDOW_HEALTH_DTYPE)


def window_health_host(sel_info: np.ndarray, sel_cap: int, windows: np.ndarray, first, requests=None, streams=None,
                       stream_samples=None):
    """window_health over host tables (bnflac_window_health_host, no GPU).  sel_info: the selection's
    FRAME_INFO_DTYPE records after the decode (at least sel_cap); windows: its WINDOW_DTYPE table;
    first: per window the position of its first record (sel_frames of select_ranges_host /
    select_windows_host, whose entries past the windows are ignored, or win_sel_first of
    select_windows_shared_host).  requests, streams, stream_samples: all None, or the requests the
    selection was made from ([(stream, first_sample[, nsamples])] or a WINDOW_REQUEST_DTYPE array), the
    STREAM_DESC_DTYPE table the scan completed and the index's stream_samples.
    -> (health[k] in WINDOW_HEALTH_DTYPE, status uint32[4])"""
    sel = np.ascontiguousarray(sel_info, dtype=FRAME_INFO_DTYPE)
    win = np.ascontiguousarray(windows, dtype=WINDOW_DTYPE)
    k = len(win)
    f = np.ascontiguousarray(first, dtype=np.uint32)
    if len(sel) < sel_cap or len(f) < k:
        raise ValueError("sel_info holds sel_cap records, first one entry per window")
    given = [x is not None for x in (requests, streams, stream_samples)]
    if any(given) and not all(given):
        raise ValueError("requests, streams and stream_samples are all given or all None")
    r = sd = ss = None
    n = 0
    if all(given):
        r = requests if isinstance(requests, np.ndarray) and requests.dtype == WINDOW_REQUEST_DTYPE else window_requests(requests)
        r = np.ascontiguousarray(r)
        sd = np.ascontiguousarray(streams, dtype=STREAM_DESC_DTYPE)
        ss = np.ascontiguousarray(stream_samples, dtype=np.uint64)
        n = len(sd)
        if len(r) != k or len(ss) != n + 1:
            raise ValueError("one request per window, and stream_samples holds nstreams + 1 entries")
    health, status = np.zeros(k, dtype=WINDOW_HEALTH_DTYPE), np.zeros(4, np.uint32)
    # a table without entries still needs an address: the call refuses null pointers
    vp = lambda a: (a if a.size else np.zeros(1, a.dtype)).ctypes.data_as(ctypes.c_void_p)
    rc = load().bnflac_window_health_host(vp(sel), sel_cap, vp(win), vp(f), k, vp(r) if r is not None else None,
                                          vp(sd) if r is not None else None, vp(ss) if r is not None else None, n,
                                          vp(health), vp(status))
    if rc != 0:
        raise RuntimeError(load().bnflac_last_error().decode())
    return health, status


FRAME_GAP = 0x800  # FRAME_INFO flags of a placeholder record of index_streams_resync
INDEX_CAND_BYTES, RESYNC_SLOT_BYTES, RESYNC_REC_BYTES = 32, 16, 32
# bnflac_index_cand: one sync candidate after the indexer's first three steps; succ and stream -1 for none
INDEX_CAND_DTYPE = np.dtype([("offset", "<u8"), ("number", "<u8"), ("succ", "<i4"), ("stream", "<i4"),
                             ("blocksize", "<u4"), ("flags", "<u4")])
CAND_VALID, CAND_SAMPLE_NUMBER = 1, 2  # INDEX_CAND flags
# bnflac_resync_slot: one record position of resync_plan_host
RESYNC_SLOT_DTYPE = np.dtype([("cand", "<u4"), ("gap", "<u4"), ("position", "<u8")])
# bnflac_resync_rec: one stream's record of index_streams_resync
RESYNC_REC_DTYPE = np.dtype([("flags", "<u4"), ("segments", "<u4"), ("gap_frames", "<u4"), ("reserved", "<u4"),
                             ("gap_samples", "<u8"), ("base", "<u8")])
assert (INDEX_CAND_DTYPE.itemsize, RESYNC_SLOT_DTYPE.itemsize, RESYNC_REC_DTYPE.itemsize) == \
    (INDEX_CAND_BYTES, RESYNC_SLOT_BYTES, RESYNC_REC_BYTES)
RESYNC_RESYNCED, RESYNC_CONTRADICTION, RESYNC_HEAD, RESYNC_LEADING = 1, 2, 4, 8  # RESYNC_REC flags


def index_cand_array(raw: np.ndarray) -> np.ndarray:
    """View a uint8 buffer of candidate records as a structured array."""
    return np.frombuffer(np.ascontiguousarray(raw).tobytes(), dtype=INDEX_CAND_DTYPE)


def resync_slot_array(raw: np.ndarray) -> np.ndarray:
    """View a uint8 buffer of resync_plan_host slots as a structured array."""
    return np.frombuffer(np.ascontiguousarray(raw).tobytes(), dtype=RESYNC_SLOT_DTYPE)


def resync_array(raw: np.ndarray) -> np.ndarray:
    """View a uint8 buffer of index_streams_resync's per-stream records as a structured array."""
    return np.frombuffer(np.ascontiguousarray(raw).tobytes(), dtype=RESYNC_REC_DTYPE)


def resync_plan_host(cands: np.ndarray, streams: np.ndarray, blocksize: int, cap: int):
    """The rule of index_streams_resync over host tables (bnflac_resync_plan_host, no GPU).  cands: an
    INDEX_CAND_DTYPE table (BatchDecoder.index_candidates gives the device's), streams: the
    STREAM_DESC_DTYPE table, blocksize: STREAMINFO's fixed blocksize, cap: the slots to provide.
    -> (slots[min(records, cap)] in RESYNC_SLOT_DTYPE, stream_frames uint32[n + 1],
        stream_samples uint64[n + 1], resync[n] in RESYNC_REC_DTYPE, status uint32[4])"""
    c = np.ascontiguousarray(cands, dtype=INDEX_CAND_DTYPE)
    sd = np.ascontiguousarray(streams, dtype=STREAM_DESC_DTYPE)
    n = len(sd)
    slots = np.zeros(max(cap, 1), dtype=RESYNC_SLOT_DTYPE)
    sf, ss = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint64)
    rec, status = np.zeros(max(n, 1), dtype=RESYNC_REC_DTYPE), np.zeros(4, np.uint32)
    vp = lambda a: (a if a.size else np.zeros(1, a.dtype)).ctypes.data_as(ctypes.c_void_p)
    rc = load().bnflac_resync_plan_host(vp(c), len(c), vp(sd), n, blocksize, vp(slots), cap, vp(sf), vp(ss), vp(rec),
                                        vp(status))
    if rc != 0:
        raise RuntimeError(load().bnflac_last_error().decode())
    return slots[: min(int(status[2]), cap)], sf, ss, rec[:n], status


def stream_table(streams, nbytes: int) -> np.ndarray:
    """The descriptor table of index_streams from [(begin, end, first_offset, total_samples)],
    checked as the library checks it (its status bit 2): ValueError for a range that is
    reversed, past nbytes, out of order or overlapping, or a first_offset outside its range."""
    table = np.zeros(len(streams), dtype=STREAM_DESC_DTYPE)
    prev_end = 0
    for k, (begin, end, first, total) in enumerate(streams):
        if not 0 <= begin <= end <= nbytes:
            raise ValueError(f"stream {k}: range [{begin}, {end}) is not inside the buffer of {nbytes} bytes")
        if not begin <= first <= end:
            raise ValueError(f"stream {k}: first_offset {first} is outside [{begin}, {end}]")
        if begin < prev_end:
            raise ValueError(f"stream {k}: range [{begin}, {end}) overlaps or precedes the previous stream's")
        if total < 0:
            raise ValueError(f"stream {k}: negative total_samples")
        prev_end = end
        table[k] = (begin, end, first, total)
    return table


def out_stride(fmt: int, sp: StreamParams) -> int:
    return int(load().bnflac_out_stride(fmt, ctypes.byref(sp)))


# bnflac_debug_last_route, word 0 (the decode) and word 6 (the parse)
RT_SYS, RT_FORK_BEFORE, RT_FORK_AFTER, RT_SERIAL, RT_SEG_ONLY, RT_W8SPLIT, RT_SW, RT_HIST = 1, 2, 4, 8, 16, 32, 64, 128
RT_PARSE_WAVE, RT_PARSE_HIST = 1, 2


def last_route() -> dict:
    """bnflac_debug_last_route as a dict: the process's last decode launch (route bits RT_*, the
    four history words it read, the launch count) and its last parse launch (k_parse_wave, whether
    the history was consulted, the hand-off mode cm, the launch count, the three words read)."""
    w = (ctypes.c_uint32 * 12)()
    load().bnflac_debug_last_route(w)
    r = int(w[0])
    return {"decode": r, "sys": bool(r & RT_SYS), "fork_before": bool(r & RT_FORK_BEFORE),
            "fork_after": bool(r & RT_FORK_AFTER), "serial": bool(r & RT_SERIAL), "seg_only": bool(r & RT_SEG_ONLY),
            "w8split": bool(r & RT_W8SPLIT), "sw": bool(r & RT_SW), "hist_read": bool(r & RT_HIST),
            "hist": tuple(int(x) for x in w[1:5]), "ndecode": int(w[5]),
            "parse_wave": bool(w[6] & RT_PARSE_WAVE), "parse_hist_read": bool(w[6] & RT_PARSE_HIST), "cm": int(w[7]),
            "nparse": int(w[8]), "parse_hist": tuple(int(x) for x in w[9:12])}


def md5_interleaved32(pcm: np.ndarray, channels: int, bps: int) -> bytes:
    """STREAMINFO md5sum of interleaved int32 PCM (host), libFLAC's byte convention."""
    a = np.ascontiguousarray(pcm, dtype=np.int32).reshape(-1)
    if a.size % channels:
        raise ValueError("pcm size is not a multiple of channels")
    out = (ctypes.c_uint8 * 16)()
    rc = load().bnflac_md5_interleaved32(a.ctypes.data if a.size else None, a.size // channels, channels, bps, out)
    if rc != 0:
        raise RuntimeError(load().bnflac_last_error().decode())
    return bytes(out)


def md5_layout(fmt: int, sp: StreamParams) -> int:
    """Bytes per sample of the MD5 message when md5_streams can hash fmt's bytes for sp, else 0."""
    return int(load().bnflac_md5_layout(fmt, ctypes.byref(sp)))


F32_MONO = 1  # gather_ranges_f32 flags: one plane per stream, the mean of the channels


def f32_layout(sp: StreamParams) -> int:
    """The narrowest layout gather_ranges_f32 accepts for sp: what decode_windows_f32 decodes into."""
    if sp.bps == 16 and sp.channels <= 2:
        return OUT_FLACDECODER
    return OUT_FILEREADER if sp.bps in (16, 24) else OUT_INTERLEAVED32


def gather_ranges_f32_host(pcm: np.ndarray, fmt: int, sp: StreamParams, windows: np.ndarray, row_samples: int,
                           mono: bool = False, plane_pitch: Optional[int] = None, pcm_bytes: Optional[int] = None):
    """gather_ranges_f32 over host memory (bnflac_gather_ranges_f32_host, no GPU).  pcm: the decoded
    bytes (uint8; read as round_up(pcm_bytes, 16) bytes, so shorter arrays are padded with zeros);
    windows: a WINDOW_DTYPE array.
    -> (float32[nstreams, planes, row_samples], status uint32[4])"""
    pcm = np.ascontiguousarray(pcm).view(np.uint8).reshape(-1)
    nbytes = pcm.size if pcm_bytes is None else min(pcm_bytes, pcm.size)
    buf = np.zeros((nbytes + 15) // 16 * 16, np.uint8)
    buf[:nbytes] = pcm[:nbytes]
    win = np.ascontiguousarray(windows, dtype=WINDOW_DTYPE)
    n = len(win)
    planes = 1 if mono else sp.channels
    pitch = row_samples if plane_pitch is None else plane_pitch
    if pitch < row_samples:
        raise ValueError("plane_pitch is below row_samples")
    out = np.zeros(max(n * planes * pitch, 1), np.float32)
    status = np.zeros(4, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
    rc = load().bnflac_gather_ranges_f32_host(vp(buf), nbytes, fmt, ctypes.byref(sp), vp(win), n, row_samples, pitch,
                                              F32_MONO if mono else 0, vp(out), vp(status))
    if rc != 0:
        raise RuntimeError(load().bnflac_last_error().decode())
    return out[: n * planes * pitch].reshape(n, planes, pitch)[:, :, :row_samples], status


class ResampleSpec(ctypes.Structure):
    """bnflac_resample_spec: rate_out / rate_in = up / down (coprime), taps per phase, and the output
    index of a window that lands in row position 0."""
    _fields_ = [("up", ctypes.c_uint32), ("down", ctypes.c_uint32), ("taps", ctypes.c_uint32),
                ("out_first", ctypes.c_uint32)]

    def with_out_first(self, out_first: int) -> "ResampleSpec":
        return ResampleSpec(self.up, self.down, self.taps, out_first)


RS_TILE = 1024  # row positions of one output tile of gather_ranges_f32_rs (csrc/bnf_resample.h)


def resample_design(rate_in: int, rate_out: int, zeros: float = 0.0, rolloff: float = 0.0, beta: float = 0.0):
    """A Kaiser-windowed sinc table for gather_ranges_f32_rs (bnflac_resample_design, no GPU); 0 for
    zeros, rolloff or beta means the default (16, 0.945, 9.0).
    -> (ResampleSpec with out_first 0, float32[up, taps]); RuntimeError for a zero rate or a table over
    the limits, with the up and taps the design needs in the message."""
    L = load()
    spec = ResampleSpec()
    need = L.bnflac_resample_design(rate_in, rate_out, zeros, rolloff, beta, ctypes.byref(spec), None, 0)
    if need < 0:
        raise RuntimeError(L.bnflac_last_error().decode())
    taps = np.zeros(need, np.float32)
    if L.bnflac_resample_design(rate_in, rate_out, zeros, rolloff, beta, ctypes.byref(spec),
                                taps.ctypes.data_as(ctypes.c_void_p), need) != need:
        raise RuntimeError(L.bnflac_last_error().decode())
    return spec, taps.reshape(spec.up, spec.taps)


def resample_request(spec: ResampleSpec, j0: int, n_out: int):
    """The source window of outputs [j0, j0 + n_out) of a stream on the output-rate grid, with the
    filter's whole support on both sides (bnflac_resample_request).
    -> (first_sample, nsamples, out_first)"""
    first, n, of = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
    if load().bnflac_resample_request(ctypes.byref(spec), j0, n_out, ctypes.byref(first), ctypes.byref(n),
                                      ctypes.byref(of)) != 0:
        raise RuntimeError(load().bnflac_last_error().decode())
    return first.value, n.value, of.value


def gather_ranges_f32_rs_host(pcm: np.ndarray, fmt: int, sp: StreamParams, windows: np.ndarray, spec: ResampleSpec,
                              taps: np.ndarray, row_out: int, mono: bool = False, plane_pitch: Optional[int] = None,
                              pcm_bytes: Optional[int] = None):
    """gather_ranges_f32_rs over host memory (bnflac_gather_ranges_f32_rs_host, no GPU).  pcm, windows:
    as for gather_ranges_f32_host; taps: float32, spec.up * spec.taps values, phase-major.
    -> (float32[nstreams, planes, row_out], status uint32[4])"""
    pcm = np.ascontiguousarray(pcm).view(np.uint8).reshape(-1)
    nbytes = pcm.size if pcm_bytes is None else min(pcm_bytes, pcm.size)
    buf = np.zeros((nbytes + 15) // 16 * 16, np.uint8)
    buf[:nbytes] = pcm[:nbytes]
    win = np.ascontiguousarray(windows, dtype=WINDOW_DTYPE)
    tab = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    if tab.size != spec.up * spec.taps:
        raise ValueError("taps holds spec.up * spec.taps values")
    n = len(win)
    planes = 1 if mono else sp.channels
    pitch = row_out if plane_pitch is None else plane_pitch
    if pitch < row_out:
        raise ValueError("plane_pitch is below row_out")
    out = np.zeros(max(n * planes * pitch, 1), np.float32)
    status = np.zeros(4, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
    rc = load().bnflac_gather_ranges_f32_rs_host(vp(buf), nbytes, fmt, ctypes.byref(sp), vp(win), n, ctypes.byref(spec),
                                                 vp(tab), row_out, pitch, F32_MONO if mono else 0, vp(out), vp(status))
    if rc != 0:
        raise RuntimeError(load().bnflac_last_error().decode())
    return out[: n * planes * pitch].reshape(n, planes, pitch)[:, :, :row_out], status


class MelSpec(ctypes.Structure):
    """bnflac_mel_spec: the FFT size, the hop, the bands (0: the power spectrum's bins), the sample
    index of tap 0 of frame 0 relative to the window, and the floats of the band weights."""
    _fields_ = [("n_fft", ctypes.c_uint32), ("hop", ctypes.c_uint32), ("n_mels", ctypes.c_uint32),
                ("origin", ctypes.c_int32), ("n_weights", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]

    @property
    def rows(self) -> int:
        return self.n_mels if self.n_mels else self.n_fft // 2 + 1

    def with_origin(self, origin: int) -> "MelSpec":
        return MelSpec(self.n_fft, self.hop, self.n_mels, origin, self.n_weights)


MEL_TILE = 32  # frames of one output tile of gather_ranges_mel (csrc/bnf_mel.h)


def mel_design(sample_rate: int, n_fft: int, hop: int, n_mels: int, f_min: float = 0.0, f_max: float = 0.0):
    """The tables of gather_ranges_mel (bnflac_mel_design, no GPU): a periodic Hann window, the
    twiddles and HTK mel triangles with their zero weights dropped; f_max 0 means sample_rate / 2,
    n_mels 0 the power spectrum.
    -> (MelSpec with origin -(n_fft // 2), tab float32[2 n_fft + n_weights], bands uint32[n_mels + 1, 2]
    or uint32[0, 2]); RuntimeError for a design over the limits, with what it needs in the message."""
    L = load()
    spec = MelSpec()
    need = L.bnflac_mel_design(sample_rate, n_fft, hop, n_mels, f_min, f_max, ctypes.byref(spec), None, 0, None, 0)
    if need < 0:
        raise RuntimeError(L.bnflac_last_error().decode())
    tab = np.zeros(need, np.float32)
    bands = np.zeros((n_mels + 1 if n_mels else 0, 2), np.uint32)
    if L.bnflac_mel_design(sample_rate, n_fft, hop, n_mels, f_min, f_max, ctypes.byref(spec),
                           tab.ctypes.data_as(ctypes.c_void_p), need,
                           bands.ctypes.data_as(ctypes.c_void_p) if bands.size else None, bands.size) != need:
        raise RuntimeError(L.bnflac_last_error().decode())
    return spec, tab, bands


def mel_to_device(mel, device):
    """(MelSpec, tab, bands) as mel_design returns them -> (MelSpec, float32 device tensor, int32 device
    tensor or None when n_mels is 0): the tables of gather_ranges_mel, uploaded once.  Tensors that
    are already on a device pass through."""
    import torch
    spec, tab, bands = mel
    if not isinstance(tab, torch.Tensor):
        tab = torch.from_numpy(np.ascontiguousarray(tab, dtype=np.float32).reshape(-1)).to(device)
    if not spec.n_mels:
        bands = None
    elif not isinstance(bands, torch.Tensor):
        bands = torch.from_numpy(np.ascontiguousarray(bands, dtype=np.uint32).reshape(-1).view(np.int32)).to(device)
    return spec, tab, bands


def mel_request(spec: MelSpec, t0: int, n_frames: int):
    """The source window of frames [t0, t0 + n_frames) of a stream's own frame grid, with the whole
    support of every frame (bnflac_mel_request).
    -> (first_sample, nsamples, origin)"""
    first, n, origin = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int32()
    if load().bnflac_mel_request(ctypes.byref(spec), t0, n_frames, ctypes.byref(first), ctypes.byref(n),
                                 ctypes.byref(origin)) != 0:
        raise RuntimeError(load().bnflac_last_error().decode())
    return first.value, n.value, origin.value


def gather_ranges_mel_host(pcm: np.ndarray, fmt: int, sp: StreamParams, windows: np.ndarray, spec: MelSpec, tab: np.ndarray,
                           bands: Optional[np.ndarray], row_frames: int, mono: bool = False,
                           frame_pitch: Optional[int] = None, pcm_bytes: Optional[int] = None):
    """gather_ranges_mel over host memory (bnflac_gather_ranges_mel_host, no GPU).  pcm, windows: as
    for gather_ranges_f32_host; tab: float32, 2 n_fft + n_weights values; bands: uint32, n_mels + 1
    pairs (None when n_mels is 0).
    -> (float32[nstreams, planes, rows, row_frames], status uint32[4])"""
    pcm = np.ascontiguousarray(pcm).view(np.uint8).reshape(-1)
    nbytes = pcm.size if pcm_bytes is None else min(pcm_bytes, pcm.size)
    buf = np.zeros((nbytes + 15) // 16 * 16, np.uint8)
    buf[:nbytes] = pcm[:nbytes]
    win = np.ascontiguousarray(windows, dtype=WINDOW_DTYPE)
    tab = np.ascontiguousarray(tab, dtype=np.float32).reshape(-1)
    if tab.size != 2 * spec.n_fft + spec.n_weights:
        raise ValueError("tab holds 2 * n_fft + n_weights values")
    bnd = np.zeros(0, np.uint32) if bands is None else np.ascontiguousarray(bands, dtype=np.uint32).reshape(-1)
    if bnd.size != (2 * (spec.n_mels + 1) if spec.n_mels else bnd.size):
        raise ValueError("bands holds n_mels + 1 pairs")
    n = len(win)
    planes = 1 if mono else sp.channels
    rows = spec.rows
    pitch = row_frames if frame_pitch is None else frame_pitch
    if pitch < row_frames:
        raise ValueError("frame_pitch is below row_frames")
    out = np.zeros(max(n * planes * rows * pitch, 1), np.float32)
    status = np.zeros(4, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
    rc = load().bnflac_gather_ranges_mel_host(vp(buf), nbytes, fmt, ctypes.byref(sp), vp(win), n, ctypes.byref(spec), vp(tab),
                                              vp(bnd), row_frames, pitch, F32_MONO if mono else 0, vp(out), vp(status))
    if rc != 0:
        raise RuntimeError(load().bnflac_last_error().decode())
    return out[: n * planes * rows * pitch].reshape(n, planes, rows, pitch)[:, :, :, :row_frames], status


def streaminfo_md5(data) -> bytes:
    """The md5sum field of a stream that starts with fLaC and its STREAMINFO block (bytes 26..42)."""
    data = bytes(data[:42])
    if len(data) < 42 or data[:4] != b"fLaC" or data[4] & 0x7F != 0:
        raise ValueError("not a FLAC stream that starts with a STREAMINFO block")
    return data[26:42]


class Corpus:
    """A batch of .flac files indexed once (BatchDecoder.index_corpus) and kept on the device:
    what decode_crops needs to cut any number of batches of crops out of it.  Nothing in it is
    written after index_corpus, so work that uses it only has to be ordered after that call (the
    same stream, or the caller's events)."""

    def __init__(self, d_bytes, nbytes, sp, nstreams, cap, d_offsets, d_info, d_stream_frames, d_stream_samples,
                 scan_status, index_status, d_streams=None, d_resync=None):
        self.d_bytes, self.nbytes, self.sp, self.nstreams, self.cap = d_bytes, nbytes, sp, nstreams, cap
        self.d_offsets, self.d_info = d_offsets, d_info
        self.d_stream_frames, self.d_stream_samples = d_stream_frames, d_stream_samples
        self.scan_status, self.index_status = scan_status, index_status  # device int32[4] each, not synchronised
        self.d_streams = d_streams  # scan_streams' descriptor table, int64[nstreams * 4], or None
        self.d_resync = d_resync  # index_streams_resync's records, uint8[nstreams * 32], or None (no resync)

    def missing_samples(self):
        """Per stream, the sample frames STREAMINFO promises and the index lacks (a damaged stream's
        chain ends at the damage): total_samples minus the samples kept, 0 where the total is 0
        (unknown, or the stream was emptied by the scan) or not above the samples kept.
        -> device int64[nstreams], not synchronised."""
        import torch
        if self.d_streams is None:
            raise ValueError("the corpus was made without the descriptor table (d_streams)")
        total = self.d_streams.view(-1)[: 4 * self.nstreams].view(self.nstreams, 4)[:, 3]
        kept = self.d_stream_samples[1: self.nstreams + 1] - self.d_stream_samples[: self.nstreams]
        return torch.where((total != 0) & (total > kept), total - kept, torch.zeros_like(total))


class BatchDecoder:
    """Device-pointer batch decode (bnflac_decode_frames) over torch CUDA tensors."""

    def __init__(self, device: int = 0):
        self.L = load()
        self.device = device
        h = ctypes.c_void_p()
        rc = self.L.bnflac_ctx_create(device, ctypes.byref(h))
        if rc != 0:
            raise RuntimeError("bnflac_ctx_create failed: " + self.L.bnflac_last_error().decode())
        self.ctx = h

    def close(self):
        if self.ctx:
            self.L.bnflac_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _stream(stream):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return ctypes.c_void_p(s.cuda_stream)

    def index_frames(self, d_bytes, nbytes: int, d_offsets, d_count, stream=None):
        rc = self.L.bnflac_index_frames(self.ctx, ctypes.c_void_p(d_bytes.data_ptr()), nbytes,
                                        ctypes.c_void_p(d_offsets.data_ptr()), d_offsets.numel(),
                                        ctypes.c_void_p(d_count.data_ptr()), self._stream(stream))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())

    def index_stream(self, d_bytes, nbytes: int, first_offset: int, sp: StreamParams, cap: int, stream=None):
        """Frame chain of a whole stream in HBM (bnflac_index_stream).
        -> (d_offsets int64[cap], d_out_sample int64[cap], d_info uint8[cap*128], nframes)."""
        import torch
        dev = d_bytes.device
        d_offs = torch.zeros(max(cap, 1), dtype=torch.int64, device=dev)
        d_os = torch.zeros(max(cap, 1), dtype=torch.int64, device=dev)
        d_info = torch.zeros(max(cap, 1) * FRAME_INFO_BYTES, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = self.L.bnflac_index_stream(self.ctx, ctypes.c_void_p(d_bytes.data_ptr()), nbytes, first_offset,
                                        ctypes.byref(sp), ctypes.c_void_p(d_offs.data_ptr()),
                                        ctypes.c_void_p(d_os.data_ptr()), ctypes.c_void_p(d_info.data_ptr()), cap,
                                        ctypes.c_void_p(d_n.data_ptr()), self._stream(stream))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())
        s = stream if stream is not None else torch.cuda.current_stream()
        s.synchronize()
        return d_offs, d_os, d_info, int(d_n.item())

    def index_streams(self, d_bytes, nbytes: int, streams, sp: StreamParams, cap: int, cand_cap: int = 0, stream=None):
        """Frame chains of many streams held in one buffer (bnflac_index_streams), one call.
        streams: [(begin, end, first_offset, total_samples)], ascending and non-overlapping, or the
        same table on the device (int64, 4 words per stream: what scan_streams returns).
        -> (d_offsets int64[cap], d_out_sample int64[cap], d_info uint8[cap*128],
            d_stream_frames int32[n+1], d_stream_samples int64[n+1], d_status int32[4]),
        all on the device and not synchronised: the caller does that, as for decode_parsed."""
        return self._index_streams(d_bytes, nbytes, streams, sp, cap, cand_cap, stream, False)

    def index_streams_resync(self, d_bytes, nbytes: int, streams, sp: StreamParams, cap: int, cand_cap: int = 0,
                             stream=None):
        """index_streams with resynchronisation (bnflac_index_streams_resync): a fixed-blocksize stream's
        chain goes on behind its damage, placeholder records (flags FRAME_GAP) hold the lost samples,
        and every later call takes the tables unchanged.  ValueError unless sp has STREAMINFO with
        min_blocksize == max_blocksize >= 1.
        -> index_streams' tuple plus d_resync uint8[n * 32] (resync_array), not synchronised."""
        if not sp.has_stream_info or sp.min_blocksize != sp.max_blocksize or sp.min_blocksize < 1:
            raise ValueError("index_streams_resync needs a fixed-blocksize stream: STREAMINFO with min_blocksize == max_blocksize")
        return self._index_streams(d_bytes, nbytes, streams, sp, cap, cand_cap, stream, True)

    def index_candidates(self) -> np.ndarray:
        """Debug: the candidate table of the last index_streams_resync call, synchronously
        (bnflac_debug_index_candidates) -> INDEX_CAND_DTYPE[ncand]."""
        n = ctypes.c_uint32(0)
        if self.L.bnflac_debug_index_candidates(self.ctx, None, 0, ctypes.byref(n)) != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())
        out = np.zeros(max(n.value, 1), dtype=INDEX_CAND_DTYPE)
        if self.L.bnflac_debug_index_candidates(self.ctx, out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)) != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())
        return out[: n.value]

    def _index_streams(self, d_bytes, nbytes, streams, sp, cap, cand_cap, stream, resync):
        import torch
        dev = d_bytes.device
        s = stream if stream is not None else torch.cuda.current_stream()
        on_device = isinstance(streams, torch.Tensor)
        if on_device:  # scan_streams' table: checked by the library (status bit 2), never read here
            d_tab, n = self._device_table(streams)
        else:
            table = stream_table(streams, nbytes)
            n = len(table)
        with torch.cuda.stream(s):
            if not on_device:
                d_tab = torch.from_numpy(table.view(np.int64).reshape(-1)).to(dev) if n else None
            d_offs = torch.zeros(max(cap, 1), dtype=torch.int64, device=dev)
            d_os = torch.zeros(max(cap, 1), dtype=torch.int64, device=dev)
            d_info = torch.zeros(max(cap, 1) * FRAME_INFO_BYTES, dtype=torch.uint8, device=dev)
            d_sf = torch.zeros(n + 1, dtype=torch.int32, device=dev)
            d_ss = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            d_status = torch.zeros(4, dtype=torch.int32, device=dev)
            d_rs = torch.zeros(max(n, 1) * RESYNC_REC_BYTES, dtype=torch.uint8, device=dev) if resync else None
        head = (self.ctx, ctypes.c_void_p(d_bytes.data_ptr()), nbytes, ctypes.c_void_p(d_tab.data_ptr()) if n else None, n,
                ctypes.byref(sp), cand_cap, ctypes.c_void_p(d_offs.data_ptr()), ctypes.c_void_p(d_os.data_ptr()),
                ctypes.c_void_p(d_info.data_ptr()), cap, ctypes.c_void_p(d_sf.data_ptr()), ctypes.c_void_p(d_ss.data_ptr()))
        tail = (ctypes.c_void_p(d_status.data_ptr()), self._stream(s))
        if resync:
            rc = self.L.bnflac_index_streams_resync(*head, ctypes.c_void_p(d_rs.data_ptr()), *tail)
        else:
            rc = self.L.bnflac_index_streams(*head, *tail)
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())
        if resync:
            return d_offs, d_os, d_info, d_sf, d_ss, d_status, d_rs[: n * RESYNC_REC_BYTES]
        return d_offs, d_os, d_info, d_sf, d_ss, d_status

    @staticmethod
    def _device_table(t):
        """A descriptor table already on the device: 4 64-bit words per stream -> (tensor, nstreams)"""
        if not t.is_cuda or t.element_size() != 8 or t.numel() % 4 or not t.is_contiguous():
            raise ValueError("a device stream table is a contiguous CUDA tensor of 4 64-bit words per stream")
        return t, t.numel() // 4

    def scan_streams(self, d_bytes, nbytes: int, ranges, expect: Optional[StreamParams] = None, stream=None):
        """The metadata of many streams held in one buffer, read on the device (bnflac_scan_streams).
        ranges: [(begin, end)], ascending and non-overlapping, or a device table (int64, 4 words per
        stream, begin and end filled in), which is completed in place and returned.
        expect: the parameters every kept stream has (a stream with others is emptied), or None.
        -> (d_table int64[n*4] ready for index_streams, d_meta uint8[n*64], d_md5 uint8[n, 16] ready
            as md5_streams' d_expected, d_status int32[4]), all on the device and not synchronised,
        like index_streams."""
        import torch
        dev = d_bytes.device
        s = stream if stream is not None else torch.cuda.current_stream()
        on_device = isinstance(ranges, torch.Tensor)
        if on_device:
            d_tab, n = self._device_table(ranges)
        else:
            n = len(ranges)
            table = np.zeros(n, dtype=STREAM_DESC_DTYPE)
            for k, (begin, end) in enumerate(ranges):
                table[k] = (begin, end, 0, 0)
        with torch.cuda.stream(s):
            if not on_device:
                d_tab = torch.from_numpy(table.view(np.int64).reshape(-1)).to(dev)
            d_meta = torch.zeros(n * STREAM_META_BYTES, dtype=torch.uint8, device=dev)
            d_md5 = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
            d_status = torch.zeros(4, dtype=torch.int32, device=dev)
        rc = self.L.bnflac_scan_streams(self.ctx, ctypes.c_void_p(d_bytes.data_ptr()), nbytes,
                                        ctypes.c_void_p(d_tab.data_ptr()) if n else None, n,
                                        ctypes.byref(expect) if expect is not None else None,
                                        ctypes.c_void_p(d_meta.data_ptr()) if n else None,
                                        ctypes.c_void_p(d_md5.data_ptr()) if n else None,
                                        ctypes.c_void_p(d_status.data_ptr()), self._stream(s))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())
        return d_tab, d_meta, d_md5, d_status

    def decode_frames(self, d_bytes, nbytes: int, d_offsets, nframes: int, sp: StreamParams, fmt: int, d_out,
                      d_info, d_out_sample=None, base_sample: int = 0, stream=None, out_bytes=None):
        """out_bytes: the output size passed to the library (default: all of d_out)"""
        nout = d_out.numel() * d_out.element_size()
        rc = self.L.bnflac_decode_frames(
            self.ctx, ctypes.c_void_p(d_bytes.data_ptr()), nbytes, ctypes.c_void_p(d_offsets.data_ptr()), nframes,
            ctypes.byref(sp), ctypes.c_void_p(d_out_sample.data_ptr()) if d_out_sample is not None else None,
            base_sample, fmt, ctypes.c_void_p(d_out.data_ptr()), nout if out_bytes is None else min(out_bytes, nout),
            ctypes.c_void_p(d_info.data_ptr()), self._stream(stream))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())


    def parse_frames(self, d_bytes, nbytes: int, d_offsets, nframes: int, sp: StreamParams, d_info,
                     d_out_sample=None, base_sample: int = 0, stream=None):
        rc = self.L.bnflac_parse_frames(
            self.ctx, ctypes.c_void_p(d_bytes.data_ptr()), nbytes, ctypes.c_void_p(d_offsets.data_ptr()), nframes,
            ctypes.byref(sp), ctypes.c_void_p(d_out_sample.data_ptr()) if d_out_sample is not None else None,
            base_sample, ctypes.c_void_p(d_info.data_ptr()), self._stream(stream))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())

    def decode_parsed(self, d_bytes, nbytes: int, nframes: int, sp: StreamParams, fmt: int, d_out, d_info,
                      stream=None):
        rc = self.L.bnflac_decode_parsed(self.ctx, ctypes.c_void_p(d_bytes.data_ptr()), nbytes, nframes,
                                         ctypes.byref(sp), fmt, ctypes.c_void_p(d_out.data_ptr()),
                                         d_out.numel() * d_out.element_size(), ctypes.c_void_p(d_info.data_ptr()),
                                         self._stream(stream))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())

    def md5_streams(self, d_pcm, fmt: int, sp: StreamParams, d_stream_samples, nstreams: int, d_expected=None,
                    stream=None, pcm_bytes=None):
        """STREAMINFO md5sum of every stream of a decoded batch, on the device (bnflac_md5_streams).
        d_stream_samples: int64[nstreams + 1] sample-frame bounds (index_streams' d_stream_samples);
        d_expected: uint8[nstreams * 16] or None; pcm_bytes: the decoded size (default: all of d_pcm).
        -> (d_md5 uint8[n, 16], d_verdict int32[n], d_status int32[4]), all on the device and not
        synchronised, like index_streams."""
        import torch
        dev = d_pcm.device
        s = stream if stream is not None else torch.cuda.current_stream()
        nbytes = d_pcm.numel() * d_pcm.element_size()
        if d_stream_samples.numel() < nstreams + 1 or d_stream_samples.element_size() != 8:
            raise ValueError("d_stream_samples must hold nstreams + 1 64-bit bounds")
        if d_expected is not None and d_expected.numel() * d_expected.element_size() < 16 * nstreams:
            raise ValueError("d_expected must hold 16 bytes per stream")
        with torch.cuda.stream(s):
            d_md5 = torch.zeros((nstreams, 16), dtype=torch.uint8, device=dev)
            d_verdict = torch.zeros(nstreams, dtype=torch.int32, device=dev)
            d_status = torch.zeros(4, dtype=torch.int32, device=dev)
        rc = self.L.bnflac_md5_streams(self.ctx, ctypes.c_void_p(d_pcm.data_ptr()),
                                       nbytes if pcm_bytes is None else min(pcm_bytes, nbytes), fmt, ctypes.byref(sp),
                                       ctypes.c_void_p(d_stream_samples.data_ptr()), nstreams,
                                       ctypes.c_void_p(d_expected.data_ptr()) if d_expected is not None else None,
                                       ctypes.c_void_p(d_md5.data_ptr()), ctypes.c_void_p(d_verdict.data_ptr()),
                                       ctypes.c_void_p(d_status.data_ptr()), self._stream(s))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())
        return d_md5, d_verdict, d_status

    def select_ranges(self, d_offsets, d_info, cap: int, d_stream_frames, d_stream_samples, nstreams: int, ranges,
                      sel_cap: int, stream=None):
        """Cut index_streams' tables down to the frames one sample window per stream needs
        (bnflac_select_ranges).  d_offsets (or None), d_info, cap, d_stream_frames, d_stream_samples:
        index_streams' outputs and its cap.  ranges: [(first_sample, nsamples)] per stream
        (TO_THE_END: up to the stream's end), or the same on the device (64-bit, 2 words per stream).
        -> (d_sel_offsets int64[sel_cap], d_sel_info uint8[sel_cap*128] ready for
            decode_parsed(nframes=sel_cap), d_sel_frames int32[n+1], d_sel_samples int64[n+1],
            d_windows uint8[n*32] for gather_ranges, d_status int32[4]),
        all on the device and not synchronised, like index_streams."""
        import torch
        dev = d_info.device
        s = stream if stream is not None else torch.cuda.current_stream()
        on_device = isinstance(ranges, torch.Tensor)
        if on_device:
            if not ranges.is_cuda or ranges.element_size() != 8 or ranges.numel() != 2 * nstreams or not ranges.is_contiguous():
                raise ValueError("device windows are a contiguous CUDA tensor of 2 64-bit words per stream")
            d_ranges = ranges
        else:
            table = sample_ranges(ranges)
            if len(table) != nstreams:
                raise ValueError("one window per stream")
        with torch.cuda.stream(s):
            if not on_device:
                d_ranges = torch.from_numpy(table.view(np.int64).reshape(-1)).to(dev) if nstreams else None
            d_sel_offs = torch.zeros(max(sel_cap, 1), dtype=torch.int64, device=dev)
            d_sel_info = torch.zeros(max(sel_cap, 1) * FRAME_INFO_BYTES, dtype=torch.uint8, device=dev)
            d_sel_f = torch.zeros(nstreams + 1, dtype=torch.int32, device=dev)
            d_sel_s = torch.zeros(nstreams + 1, dtype=torch.int64, device=dev)
            d_win = torch.zeros(max(nstreams, 1) * WINDOW_BYTES, dtype=torch.uint8, device=dev)
            d_status = torch.zeros(4, dtype=torch.int32, device=dev)
        vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = self.L.bnflac_select_ranges(self.ctx, vp(d_offsets), vp(d_info), cap, vp(d_stream_frames),
                                         vp(d_stream_samples), nstreams, vp(d_ranges) if nstreams else None,
                                         vp(d_sel_offs) if d_offsets is not None else None, vp(d_sel_info), sel_cap,
                                         vp(d_sel_f), vp(d_sel_s), vp(d_win), vp(d_status), self._stream(s))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())
        return d_sel_offs, d_sel_info, d_sel_f, d_sel_s, d_win, d_status

    def select_windows(self, d_offsets, d_info, cap: int, d_stream_frames, d_stream_samples, nstreams: int, requests,
                       sel_cap: int, stream=None):
        """Cut index_streams' tables down to the frames any crops of the batch need
        (bnflac_select_windows): select_ranges with one output row per request instead of per stream.
        requests: [(stream, first_sample[, nsamples])], any number per stream in any order, or the
        same on the device (a contiguous 64-bit tensor of 3 words per window).  The tables are only
        read.
        -> (d_sel_offsets int64[sel_cap], d_sel_info uint8[sel_cap*128] ready for
            decode_parsed(nframes=sel_cap), d_sel_frames int32[k+1], d_sel_samples int64[k+1],
            d_windows uint8[k*32] for gather_ranges(nstreams=k), d_status int32[4]) for k requests,
        all on the device and not synchronised, like select_ranges."""
        import torch
        dev = d_info.device
        s = stream if stream is not None else torch.cuda.current_stream()
        on_device = isinstance(requests, torch.Tensor)
        if on_device:
            if not requests.is_cuda or requests.element_size() != 8 or requests.numel() % 3 or not requests.is_contiguous():
                raise ValueError("device requests are a contiguous CUDA tensor of 3 64-bit words per window")
            d_req, k = requests, requests.numel() // 3
        else:
            table = window_requests(requests)
            k = len(table)
        with torch.cuda.stream(s):
            if not on_device:
                d_req = torch.from_numpy(table.view(np.int64).reshape(-1)).to(dev) if k else None
            d_sel_offs = torch.zeros(max(sel_cap, 1), dtype=torch.int64, device=dev)
            d_sel_info = torch.zeros(max(sel_cap, 1) * FRAME_INFO_BYTES, dtype=torch.uint8, device=dev)
            d_sel_f = torch.zeros(k + 1, dtype=torch.int32, device=dev)
            d_sel_s = torch.zeros(k + 1, dtype=torch.int64, device=dev)
            d_win = torch.zeros(max(k, 1) * WINDOW_BYTES, dtype=torch.uint8, device=dev)
            d_status = torch.zeros(4, dtype=torch.int32, device=dev)
        vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = self.L.bnflac_select_windows(self.ctx, vp(d_offsets), vp(d_info), cap, vp(d_stream_frames),
                                          vp(d_stream_samples), nstreams, vp(d_req) if k else None, k,
                                          vp(d_sel_offs) if d_offsets is not None else None, vp(d_sel_info), sel_cap,
                                          vp(d_sel_f), vp(d_sel_s), vp(d_win), vp(d_status), self._stream(s))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())
        return d_sel_offs, d_sel_info, d_sel_f, d_sel_s, d_win, d_status

    def select_windows_shared(self, d_offsets, d_info, cap: int, d_stream_frames, d_stream_samples, nstreams: int,
                              requests, sel_cap: int, stream=None):
        """select_windows for crops that overlap (bnflac_select_windows_shared): the union of the
        frames the requests need, each selected once, and windows that point into the one compact
        PCM those frames decode into.  Arguments as for select_windows; the scratch kept in the
        context grows by 16 bytes per position of cap.
        -> (d_sel_offsets int64[sel_cap], d_sel_info uint8[sel_cap*128] ready for
            decode_parsed(nframes=sel_cap), d_windows uint8[k*32] for gather_ranges(nstreams=k),
            d_win_sel_first int32[k], d_totals int64[2] = (frames, samples), d_status int32[4]) for k
        requests, all on the device and not synchronised."""
        import torch
        dev = d_info.device
        s = stream if stream is not None else torch.cuda.current_stream()
        on_device = isinstance(requests, torch.Tensor)
        if on_device:
            if not requests.is_cuda or requests.element_size() != 8 or requests.numel() % 3 or not requests.is_contiguous():
                raise ValueError("device requests are a contiguous CUDA tensor of 3 64-bit words per window")
            d_req, k = requests, requests.numel() // 3
        else:
            table = window_requests(requests)
            k = len(table)
        with torch.cuda.stream(s):
            if not on_device:
                d_req = torch.from_numpy(table.view(np.int64).reshape(-1)).to(dev) if k else None
            d_sel_offs = torch.zeros(max(sel_cap, 1), dtype=torch.int64, device=dev)
            d_sel_info = torch.zeros(max(sel_cap, 1) * FRAME_INFO_BYTES, dtype=torch.uint8, device=dev)
            d_win = torch.zeros(max(k, 1) * WINDOW_BYTES, dtype=torch.uint8, device=dev)
            d_first = torch.zeros(max(k, 1), dtype=torch.int32, device=dev)
            d_totals = torch.zeros(2, dtype=torch.int64, device=dev)
            d_status = torch.zeros(4, dtype=torch.int32, device=dev)
        vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = self.L.bnflac_select_windows_shared(self.ctx, vp(d_offsets), vp(d_info), cap, vp(d_stream_frames),
                                                 vp(d_stream_samples), nstreams, vp(d_req) if k else None, k,
                                                 vp(d_sel_offs) if d_offsets is not None else None, vp(d_sel_info),
                                                 sel_cap, vp(d_win), vp(d_first), vp(d_totals), vp(d_status),
                                                 self._stream(s))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())
        return d_sel_offs, d_sel_info, d_win, d_first[:k], d_totals, d_status

    def window_health(self, d_sel_info, sel_cap: int, d_windows, d_first, nwindows: int, requests=None, corpus=None,
                      stream=None):
        """Which windows of a decoded selection hold damaged or missing audio (bnflac_window_health),
        after decode_parsed on the same stream.  d_sel_info, sel_cap, d_windows: the selection's records
        and window table; d_first: the position of each window's first record, d_sel_frames of
        select_ranges / select_windows or d_win_sel_first of select_windows_shared.
        requests, corpus: both None (bad frames only: missing is 0, SHORT and NO_STREAM are never
        set), or the requests the selection was made from ([(stream, first_sample[, nsamples])] or a
        device tensor of 3 64-bit words per window) and the Corpus they name streams of, whose
        descriptor table and sample bounds say what STREAMINFO promises and what the index kept.
        -> (d_health uint8[nwindows * 32] for health_array, d_status int32[4]: bit 0 / 1 / 2 of word 0
            some window DAMAGED / SHORT / UNKNOWN, then how many of each), on the device and not
        synchronised."""
        import torch
        dev = d_sel_info.device
        s = stream if stream is not None else torch.cuda.current_stream()
        if (requests is None) != (corpus is None):
            raise ValueError("requests and corpus are both given or both None")
        d_req = d_streams = d_ss = None
        nstreams = 0
        if requests is not None:
            if corpus.d_streams is None:
                raise ValueError("the corpus was made without the descriptor table (d_streams)")
            d_streams, d_ss, nstreams = corpus.d_streams, corpus.d_stream_samples, corpus.nstreams
            if isinstance(requests, torch.Tensor):
                if not requests.is_cuda or requests.element_size() != 8 or requests.numel() % 3 or not requests.is_contiguous():
                    raise ValueError("device requests are a contiguous CUDA tensor of 3 64-bit words per window")
                d_req, k = requests, requests.numel() // 3
            else:
                table = window_requests(requests)
                k = len(table)
            if k != nwindows:
                raise ValueError("one request per window")
        if d_first.numel() < nwindows or d_first.element_size() != 4:
            raise ValueError("d_first holds one 32-bit position per window")
        with torch.cuda.stream(s):
            if requests is not None:
                if d_req is None:
                    d_req = torch.from_numpy(table.view(np.int64).reshape(-1)).to(dev)
                # a table without entries still needs an address: the three are all given or all null
                some = lambda t: t if t.numel() else torch.zeros(1, dtype=torch.int64, device=dev)
                d_req, d_streams = some(d_req), some(d_streams)
            d_health = torch.zeros(max(nwindows, 1) * WINDOW_HEALTH_BYTES, dtype=torch.uint8, device=dev)
            d_status = torch.zeros(4, dtype=torch.int32, device=dev)
        vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = self.L.bnflac_window_health(self.ctx, vp(d_sel_info), sel_cap, vp(d_windows), vp(d_first), nwindows,
                                         vp(d_req), vp(d_streams), vp(d_ss), nstreams, vp(d_health), vp(d_status),
                                         self._stream(s))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())
        return d_health[: nwindows * WINDOW_HEALTH_BYTES], d_status

    def gather_ranges(self, d_pcm, fmt: int, sp: StreamParams, d_windows, nstreams: int, row_samples: int,
                      row_bytes: Optional[int] = None, d_rows=None, stream=None, pcm_bytes=None):
        """The windows of a decoded selection as rows of one shape (bnflac_gather_ranges): row s is
        min(window s's nsamples, row_samples) sample frames of d_pcm from its pcm_first, then zeros.
        row_bytes: the distance between rows (default: row_samples * stride); d_rows: the output
        (default: a new uint8 tensor of nstreams * row_bytes, whose bytes between rows are zero);
        pcm_bytes: the decoded size (default: all of d_pcm).
        -> (d_rows, d_status int32[4]), on the device and not synchronised."""
        import torch
        dev = d_pcm.device
        s = stream if stream is not None else torch.cuda.current_stream()
        nbytes = d_pcm.numel() * d_pcm.element_size()
        width = row_samples * out_stride(fmt, sp)
        row_bytes = width if row_bytes is None else row_bytes
        with torch.cuda.stream(s):
            if d_rows is None:
                d_rows = torch.zeros(max(nstreams * row_bytes, 1), dtype=torch.uint8, device=dev)
            d_status = torch.zeros(4, dtype=torch.int32, device=dev)
        if nstreams and d_rows.numel() * d_rows.element_size() < (nstreams - 1) * row_bytes + width:
            raise ValueError("d_rows is too small for nstreams rows")
        rc = self.L.bnflac_gather_ranges(self.ctx, ctypes.c_void_p(d_pcm.data_ptr()),
                                         nbytes if pcm_bytes is None else min(pcm_bytes, nbytes), fmt, ctypes.byref(sp),
                                         ctypes.c_void_p(d_windows.data_ptr()), nstreams, row_samples, row_bytes,
                                         ctypes.c_void_p(d_rows.data_ptr()), ctypes.c_void_p(d_status.data_ptr()),
                                         self._stream(s))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())
        return d_rows, d_status

    def decode_windows(self, d_bytes, nbytes: int, ranges_bytes, windows, nsamples: int, sp: StreamParams, fmt: int,
                       cap: Optional[int] = None, cand_cap: int = 0, stream=None):
        """nsamples sample frames from a position of its own in every .flac file of a buffer:
        scan_streams -> index_streams -> select_ranges -> decode_parsed(nframes = sel_cap) ->
        gather_ranges, with no host synchronisation and nothing read back.
        ranges_bytes: the files, as for scan_streams; sp: the parameters every file must have (others
        are emptied by the scan and give zero rows); windows: one first sample per stream, or
        [(first_sample, n)] with n <= nsamples, or a device tensor of 2 64-bit words per stream;
        cap, cand_cap: as for index_streams (cap defaults to nbytes // 16 + 16).
        Sizes, for n = nsamples >= 1: sel_cap = nstreams * ((n - 1) // min_blocksize + 2) records (only
        a stream's last frame may be shorter than min_blocksize) and a compact PCM of
        nstreams * (n + 2 * (max_blocksize - 1)) sample frames.  A stream whose STREAMINFO understates
        its frames shows up as bit 0 of the select status (and its row may be zero), not as a fault.
        -> (rows, status): rows int32[nstreams, nsamples, channels] for OUT_INTERLEAVED32, else
        uint8[nstreams, nsamples * stride]; status: the device status words of each stage,
        {"scan", "index", "select", "gather"} -> int32[4]."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        d_pcm, d_win, n, status = self._decode_selection(d_bytes, nbytes, ranges_bytes, windows, nsamples, sp, fmt, cap,
                                                         cand_cap, s)
        stride = out_stride(fmt, sp)
        d_rows, status["gather"] = self.gather_ranges(d_pcm, fmt, sp, d_win, n, nsamples, stream=s)
        with torch.cuda.stream(s):
            if fmt == OUT_INTERLEAVED32:
                rows = d_rows[: n * nsamples * stride].view(torch.int32).view(n, nsamples, sp.channels)
            else:
                rows = d_rows[: n * nsamples * stride].view(n, nsamples * stride)
        return rows, status

    def _decode_selection(self, d_bytes, nbytes, ranges_bytes, windows, nsamples, sp, fmt, cap, cand_cap, s):
        """The front of decode_windows and decode_windows_f32: scan_streams -> index_streams ->
        select_ranges -> decode_parsed(nframes = sel_cap) into a compact PCM in fmt, on stream s.
        -> (d_pcm, d_windows, nstreams, {"scan", "index", "select"} -> int32[4])"""
        import torch
        if nsamples < 1:
            raise ValueError("nsamples must be at least 1")
        if fmt == OUT_PLANAR32:
            raise ValueError("OUT_PLANAR32 is channel-major per frame: a window of it is no byte range")
        if sp.min_blocksize < 1 or sp.max_blocksize < sp.min_blocksize:
            raise ValueError("sp must carry STREAMINFO's min_blocksize and max_blocksize")
        dev = d_bytes.device
        n = ranges_bytes.numel() // 4 if isinstance(ranges_bytes, torch.Tensor) else len(ranges_bytes)
        if not isinstance(windows, torch.Tensor):
            windows = [(w, nsamples) if np.isscalar(w) else tuple(w) for w in windows]
        cap = nbytes // 16 + 16 if cap is None else cap
        sel_cap = n * ((nsamples - 1) // sp.min_blocksize + 2)
        stride = out_stride(fmt, sp)
        d_tab, _, _, st_scan = self.scan_streams(d_bytes, nbytes, ranges_bytes, expect=sp, stream=s)
        d_offs, _, d_info, d_sf, d_ss, st_index = self.index_streams(d_bytes, nbytes, d_tab, sp, cap, cand_cap=cand_cap,
                                                                     stream=s)
        _, d_sel_info, _, _, d_win, st_select = self.select_ranges(d_offs, d_info, cap, d_sf, d_ss, n, windows, sel_cap,
                                                                   stream=s)
        with torch.cuda.stream(s):
            pcm_bytes = n * (nsamples + 2 * (sp.max_blocksize - 1)) * stride
            d_pcm = torch.zeros(max((pcm_bytes + 15) // 16 * 16, 16), dtype=torch.uint8, device=dev)
        self.decode_parsed(d_bytes, nbytes, sel_cap, sp, fmt, d_pcm, d_sel_info, stream=s)
        return d_pcm, d_win, n, {"scan": st_scan, "index": st_index, "select": st_select}

    def gather_ranges_f32(self, d_pcm, fmt: int, sp: StreamParams, d_windows, nstreams: int, row_samples: int,
                          mono: bool = False, d_out=None, plane_pitch: Optional[int] = None, stream=None, pcm_bytes=None):
        """The windows of a decoded selection as normalised float32 channel planes
        (bnflac_gather_ranges_f32): plane c of stream s is min(window s's nsamples, row_samples)
        samples of channel c from its pcm_first, as sample * 2^-(bps - 1), then zeros; mono: one plane,
        the mean of the channels.  fmt: a layout md5_layout accepts for sp (f32_layout(sp) is the
        narrowest).  plane_pitch: floats between planes (default: row_samples); d_out: the output, a
        float32 tensor (default: a new one); pcm_bytes: the decoded size (default: all of d_pcm).
        -> (float32[nstreams, planes, row_samples], a view of d_out when one is passed; d_status int32[4]),
        on the device and not synchronised."""
        import torch
        dev = d_pcm.device
        s = stream if stream is not None else torch.cuda.current_stream()
        nbytes = d_pcm.numel() * d_pcm.element_size()
        planes = 1 if mono else sp.channels
        pitch = row_samples if plane_pitch is None else plane_pitch
        if pitch < row_samples:
            raise ValueError("plane_pitch is below row_samples")
        with torch.cuda.stream(s):
            if d_out is None:
                d_out = torch.zeros(max(nstreams * planes * pitch, 1), dtype=torch.float32, device=dev)
            d_status = torch.zeros(4, dtype=torch.int32, device=dev)
        if d_out.dtype != torch.float32 or not d_out.is_contiguous():
            raise ValueError("d_out is a contiguous float32 tensor")
        if nstreams and d_out.numel() < (nstreams * planes - 1) * pitch + row_samples:
            raise ValueError("d_out is too small for nstreams * planes planes")
        rc = self.L.bnflac_gather_ranges_f32(self.ctx, ctypes.c_void_p(d_pcm.data_ptr()),
                                             nbytes if pcm_bytes is None else min(pcm_bytes, nbytes), fmt, ctypes.byref(sp),
                                             ctypes.c_void_p(d_windows.data_ptr()), nstreams, row_samples, pitch,
                                             F32_MONO if mono else 0, ctypes.c_void_p(d_out.data_ptr()),
                                             ctypes.c_void_p(d_status.data_ptr()), self._stream(s))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())
        planes_view = torch.as_strided(d_out.view(-1), (nstreams, planes, row_samples), (planes * pitch, pitch, 1))
        return planes_view, d_status

    def decode_windows_f32(self, d_bytes, nbytes: int, ranges_bytes, windows, nsamples: int, sp: StreamParams,
                           fmt: Optional[int] = None, mono: bool = False, cap: Optional[int] = None, cand_cap: int = 0,
                           stream=None):
        """decode_windows with gather_ranges_f32 as its last step: nsamples sample frames from a
        position of its own in every .flac file of a buffer, as float32 channel planes in [-1, 1),
        with no host synchronisation and nothing read back.  Arguments, sizes and the status
        dictionary are decode_windows' ("gather" is gather_ranges_f32's status).  fmt: the layout the
        frames decode into, None for the narrowest one gather_ranges_f32 accepts (f32_layout(sp):
        OUT_FLACDECODER for 16-bit streams of 1-2 channels, else OUT_FILEREADER for 16- and 24-bit
        streams, else OUT_INTERLEAVED32).  mono: one plane per stream, the mean of the channels.
        -> (float32[nstreams, planes, nsamples], status)"""
        import torch
        fmt = f32_layout(sp) if fmt is None else fmt
        if not md5_layout(fmt, sp):
            raise ValueError("the layout's bytes are not the samples: gather_ranges_f32 cannot read it")
        s = stream if stream is not None else torch.cuda.current_stream()
        d_pcm, d_win, n, status = self._decode_selection(d_bytes, nbytes, ranges_bytes, windows, nsamples, sp, fmt, cap,
                                                         cand_cap, s)
        planes, status["gather"] = self.gather_ranges_f32(d_pcm, fmt, sp, d_win, n, nsamples, mono=mono, stream=s)
        return planes, status

    def index_corpus(self, d_bytes, nbytes: int, ranges_bytes, sp: StreamParams, cap: Optional[int] = None,
                     cand_cap: int = 0, stream=None, resync: bool = False) -> Corpus:
        """scan_streams -> index_streams over the .flac files of a buffer, once, for any number of
        decode_crops / decode_crops_f32 calls.  Arguments as for decode_windows (cap defaults to
        nbytes // 16 + 16); nothing is synchronised or read back.  The caller keeps d_bytes alive and
        unchanged as long as the Corpus is used, and orders that use after this call (the same
        stream, or events).
        resync: index_streams_resync in index_streams' place (fixed-blocksize streams; ValueError when
        sp.min_blocksize != sp.max_blocksize): a damaged stream loses its damaged frames only, whose
        samples come back as zeros in a crop that window_health calls DAMAGED; Corpus.d_resync holds
        the per-stream records (None without resync)."""
        import torch
        if resync and sp.min_blocksize != sp.max_blocksize:
            raise ValueError("resync needs a fixed-blocksize stream: sp.min_blocksize != sp.max_blocksize")
        s = stream if stream is not None else torch.cuda.current_stream()
        n = ranges_bytes.numel() // 4 if isinstance(ranges_bytes, torch.Tensor) else len(ranges_bytes)
        cap = nbytes // 16 + 16 if cap is None else cap
        d_tab, _, _, st_scan = self.scan_streams(d_bytes, nbytes, ranges_bytes, expect=sp, stream=s)
        d_rs = None
        if resync:
            d_offs, _, d_info, d_sf, d_ss, st_index, d_rs = self.index_streams_resync(d_bytes, nbytes, d_tab, sp, cap,
                                                                                      cand_cap=cand_cap, stream=s)
        else:
            d_offs, _, d_info, d_sf, d_ss, st_index = self.index_streams(d_bytes, nbytes, d_tab, sp, cap, cand_cap=cand_cap,
                                                                         stream=s)
        return Corpus(d_bytes, nbytes, sp, n, cap, d_offs, d_info, d_sf, d_ss, st_scan, st_index, d_tab, d_rs)

    def _decode_crop_selection(self, corpus: Corpus, requests, nsamples, fmt, s, shared=False, max_frames=None,
                               max_samples=None, health=False):
        """The front of decode_crops and decode_crops_f32: select_windows over the corpus's index ->
        decode_parsed(nframes = sel_cap) of the copied records into a compact PCM in fmt, on stream s.
        shared: select_windows_shared in select_windows' place, with sel_cap = max_frames and a PCM of
        max_samples sample frames where they are given, and "totals" in the status.
        health: window_health over the completed records, "health" and "windows_health" in the status;
        the requests are uploaded once, for the selection and for it.
        -> (d_pcm, d_windows, nwindows, the PCM's bytes when shared else None, {"select" -> int32[4]})"""
        import torch
        sp = corpus.sp
        if nsamples < 1:
            raise ValueError("nsamples must be at least 1")
        if fmt == OUT_PLANAR32:
            raise ValueError("OUT_PLANAR32 is channel-major per frame: a window of it is no byte range")
        if sp.min_blocksize < 1 or sp.max_blocksize < sp.min_blocksize:
            raise ValueError("sp must carry STREAMINFO's min_blocksize and max_blocksize")
        if health and corpus.d_streams is None:
            raise ValueError("health needs the corpus's descriptor table (d_streams): index_corpus keeps it")
        if isinstance(requests, torch.Tensor):
            k = requests.numel() // 3
        else:
            requests = [(r[0], r[1], nsamples) if len(r) == 2 else tuple(r) for r in requests]
            k = len(requests)
        sel_cap = k * ((nsamples - 1) // sp.min_blocksize + 2)
        pcm_samples = k * (nsamples + 2 * (sp.max_blocksize - 1))
        stride = out_stride(fmt, sp)
        status = {}
        if health and k and not isinstance(requests, torch.Tensor):
            with torch.cuda.stream(s):
                requests = torch.from_numpy(window_requests(requests).view(np.int64).reshape(-1)).to(corpus.d_bytes.device)
        if shared:  # the union is never larger than the sum, nor than the index
            sel_cap = min(sel_cap, corpus.cap) if max_frames is None else max_frames
            pcm_samples = pcm_samples if max_samples is None else max_samples
            if sel_cap < 0 or pcm_samples < 0:
                raise ValueError("max_frames and max_samples are counts")
            _, d_sel_info, d_win, d_first, status["totals"], status["select"] = self.select_windows_shared(
                corpus.d_offsets, corpus.d_info, corpus.cap, corpus.d_stream_frames, corpus.d_stream_samples,
                corpus.nstreams, requests, sel_cap, stream=s)
        else:
            if max_frames is not None or max_samples is not None:
                raise ValueError("max_frames and max_samples size the shared selection: pass shared=True")
            _, d_sel_info, d_first, _, d_win, status["select"] = self.select_windows(
                corpus.d_offsets, corpus.d_info, corpus.cap, corpus.d_stream_frames, corpus.d_stream_samples,
                corpus.nstreams, requests, sel_cap, stream=s)
        with torch.cuda.stream(s):
            pcm_bytes = pcm_samples * stride
            d_pcm = torch.zeros(max((pcm_bytes + 15) // 16 * 16, 16), dtype=torch.uint8, device=corpus.d_bytes.device)
        self.decode_parsed(corpus.d_bytes, corpus.nbytes, sel_cap, sp, fmt, d_pcm, d_sel_info, stream=s)
        if health:
            d_health, status["health"] = self.window_health(d_sel_info, sel_cap, d_win, d_first, k, requests, corpus,
                                                            stream=s)
            status["windows_health"] = d_health.view(k, WINDOW_HEALTH_BYTES)
        return d_pcm, d_win, k, pcm_bytes if shared else None, status

    def decode_crops(self, corpus: Corpus, requests, nsamples: int, fmt: int, stream=None, shared: bool = False,
                     max_frames: Optional[int] = None, max_samples: Optional[int] = None, health: bool = False):
        """Any crops of nsamples sample frames out of an indexed corpus, as rows in request order:
        select_windows -> decode_parsed(nframes = sel_cap) -> gather_ranges over the index that
        index_corpus made, with no host synchronisation and nothing read back.
        requests: [(stream, first_sample)] or [(stream, first_sample, n)] with n <= nsamples, any
        number per stream (a frame two crops share is decoded twice), or a device tensor of 3 64-bit
        words per crop; a stream id that is not in the corpus gives a zero row and bit 2 of the
        select status.  Sizes are decode_windows' with the crops in the streams' place: sel_cap =
        k * ((nsamples - 1) // min_blocksize + 2) records, a compact PCM of
        k * (nsamples + 2 * (max_blocksize - 1)) sample frames.  The decode completes the copied
        records, never the corpus's, so one corpus serves any number of calls; each must be ordered
        after index_corpus (the same stream, or the caller's events).
        shared: select_windows_shared in select_windows' place, for crops that overlap (sliding
        windows): every frame is selected and decoded once and the rows are the same.  max_frames,
        max_samples (shared only): the records and the sample frames of the compact PCM to provide,
        where the caller knows the union's size; the defaults are the bounds above with sel_cap no
        larger than corpus.cap, which always suffice.  Too small a max_frames shows as bit 0 of the
        select status, a crop whose samples were not provided as a zero row and the gather status.
        health: window_health after the decode, over the same uploaded requests: a frame that failed
        to decode or failed its CRC leaves zeros in a row, and a stream whose index ends at damage
        gives clipped or empty rows; the records say which crops and how many sample frames.  The
        rows and the other status entries are what health=False gives.
        -> (rows, status): rows int32[k, nsamples, channels] for OUT_INTERLEAVED32, else
        uint8[k, nsamples * stride]; status: {"select", "gather"} -> device int32[4], with
        shared "totals" -> device int64[2], the frames and sample frames selected, and with health
        "health" -> device int32[4] and "windows_health" -> device uint8[k, 32] (health_array)."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        sp = corpus.sp
        d_pcm, d_win, k, pcm_bytes, status = self._decode_crop_selection(corpus, requests, nsamples, fmt, s, shared,
                                                                         max_frames, max_samples, health)
        stride = out_stride(fmt, sp)
        d_rows, status["gather"] = self.gather_ranges(d_pcm, fmt, sp, d_win, k, nsamples, stream=s, pcm_bytes=pcm_bytes)
        with torch.cuda.stream(s):
            if fmt == OUT_INTERLEAVED32:
                rows = d_rows[: k * nsamples * stride].view(torch.int32).view(k, nsamples, sp.channels)
            else:
                rows = d_rows[: k * nsamples * stride].view(k, nsamples * stride)
        return rows, status

    def decode_crops_f32(self, corpus: Corpus, requests, nsamples: int, fmt: Optional[int] = None, mono: bool = False,
                         stream=None, shared: bool = False, max_frames: Optional[int] = None,
                         max_samples: Optional[int] = None, health: bool = False):
        """decode_crops with gather_ranges_f32 as its last step: the crops as float32 channel planes
        in [-1, 1), in request order.  fmt, mono: as for decode_windows_f32; shared, max_frames,
        max_samples, health: as for decode_crops.
        -> (float32[k, planes, nsamples], status)"""
        import torch
        sp = corpus.sp
        fmt = f32_layout(sp) if fmt is None else fmt
        if not md5_layout(fmt, sp):
            raise ValueError("the layout's bytes are not the samples: gather_ranges_f32 cannot read it")
        s = stream if stream is not None else torch.cuda.current_stream()
        d_pcm, d_win, k, pcm_bytes, status = self._decode_crop_selection(corpus, requests, nsamples, fmt, s, shared,
                                                                         max_frames, max_samples, health)
        planes, status["gather"] = self.gather_ranges_f32(d_pcm, fmt, sp, d_win, k, nsamples, mono=mono, stream=s,
                                                          pcm_bytes=pcm_bytes)
        return planes, status

    def gather_ranges_f32_rs(self, d_pcm, fmt: int, sp: StreamParams, d_windows, nstreams: int, spec: ResampleSpec, d_taps,
                             row_out: int, mono: bool = False, d_out=None, plane_pitch: Optional[int] = None, stream=None,
                             pcm_bytes=None):
        """gather_ranges_f32 with the windows filtered to another sample rate in the same launch
        (bnflac_gather_ranges_f32_rs): row position r of plane c of stream s is output r + spec.out_first
        of window s's channel c (mono: of the mean of the channels) through the polyphase FIR d_taps,
        a float32 device tensor of spec.up * spec.taps values, phase-major (resample_design makes one);
        then zeros.  The other arguments are gather_ranges_f32's, with row_out in row_samples' place.
        -> (float32[nstreams, planes, row_out], a view of d_out when one is passed; d_status int32[4]),
        on the device and not synchronised."""
        import torch
        dev = d_pcm.device
        s = stream if stream is not None else torch.cuda.current_stream()
        nbytes = d_pcm.numel() * d_pcm.element_size()
        planes = 1 if mono else sp.channels
        pitch = row_out if plane_pitch is None else plane_pitch
        if pitch < row_out:
            raise ValueError("plane_pitch is below row_out")
        if d_taps.dtype != torch.float32 or not d_taps.is_contiguous() or d_taps.numel() != spec.up * spec.taps:
            raise ValueError("d_taps is a contiguous float32 tensor of spec.up * spec.taps values")
        with torch.cuda.stream(s):
            if d_out is None:
                d_out = torch.zeros(max(nstreams * planes * pitch, 1), dtype=torch.float32, device=dev)
            d_status = torch.zeros(4, dtype=torch.int32, device=dev)
        if d_out.dtype != torch.float32 or not d_out.is_contiguous():
            raise ValueError("d_out is a contiguous float32 tensor")
        if nstreams and d_out.numel() < (nstreams * planes - 1) * pitch + row_out:
            raise ValueError("d_out is too small for nstreams * planes planes")
        rc = self.L.bnflac_gather_ranges_f32_rs(self.ctx, ctypes.c_void_p(d_pcm.data_ptr()),
                                                nbytes if pcm_bytes is None else min(pcm_bytes, nbytes), fmt,
                                                ctypes.byref(sp), ctypes.c_void_p(d_windows.data_ptr()), nstreams,
                                                ctypes.byref(spec), ctypes.c_void_p(d_taps.data_ptr()), row_out, pitch,
                                                F32_MONO if mono else 0, ctypes.c_void_p(d_out.data_ptr()),
                                                ctypes.c_void_p(d_status.data_ptr()), self._stream(s))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())
        planes_view = torch.as_strided(d_out.view(-1), (nstreams, planes, row_out), (planes * pitch, pitch, 1))
        return planes_view, d_status

    def decode_crops_f32_rs(self, corpus: Corpus, crops, n_out: int, rate_out: int, fmt: Optional[int] = None,
                            mono: bool = False, stream=None, shared: bool = True, design=None, zeros: float = 0.0,
                            rolloff: float = 0.0, beta: float = 0.0):
        """Crops of an indexed corpus at another sample rate: n_out outputs from output index j0 of a
        stream's grid at rate_out, as float32 channel planes, with no host synchronisation and nothing
        read back.  crops: [(stream, j0)], positions at the output rate.  resample_request turns every
        crop into a source window with the filter's margins, then select_windows[_shared] ->
        decode_parsed -> gather_ranges_f32_rs; shared (the default) decodes a frame once for all the
        crops whose margins overlap in it.  A crop past the stream's end is clipped by the selection
        and gives zeros there, as the whole stream resampled in one window would.
        design: (ResampleSpec, float32 taps) to use, else resample_design(corpus.sp.sample_rate,
        rate_out, zeros, rolloff, beta).  One gather launch serves the crops that share an out_first
        (all of them when every j0 is a multiple of spec.up); the crops are grouped by it.
        -> (float32[k, planes, n_out] in request order, status: decode_crops' entries, "gather" the sum
        of the groups' status words with [0] their OR)"""
        import torch
        sp = corpus.sp
        fmt = f32_layout(sp) if fmt is None else fmt
        if not md5_layout(fmt, sp):
            raise ValueError("the layout's bytes are not the samples: gather_ranges_f32_rs cannot read it")
        if n_out < 1:
            raise ValueError("n_out must be at least 1")
        s = stream if stream is not None else torch.cuda.current_stream()
        dev = corpus.d_bytes.device
        spec, taps = design if design is not None else resample_design(sp.sample_rate, rate_out, zeros, rolloff, beta)
        k = len(crops)
        planes = 1 if mono else sp.channels
        asked = [(int(t), ) + resample_request(spec, int(j0), n_out) for t, j0 in crops]  # (stream, first, n, out_first)
        order = sorted(range(k), key=lambda i: asked[i][3])
        requests = [asked[i][:3] for i in order]
        nsamples = max([r[2] for r in requests] + [1])
        d_pcm, d_win, _, pcm_bytes, status = self._decode_crop_selection(corpus, requests, nsamples, fmt, s, shared)
        pitch = (n_out + 3) // 4 * 4  # every group's first plane stays 16-byte aligned
        with torch.cuda.stream(s):
            d_taps = torch.from_numpy(np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)).to(dev)
            d_out = torch.zeros(max(k * planes * pitch, 1), dtype=torch.float32, device=dev)
        sts, g0 = [], 0
        while g0 < k:
            g1 = g0
            while g1 < k and asked[order[g1]][3] == asked[order[g0]][3]:
                g1 += 1
            _, st = self.gather_ranges_f32_rs(d_pcm, fmt, sp, d_win[g0 * WINDOW_BYTES:], g1 - g0,
                                              spec.with_out_first(asked[order[g0]][3]), d_taps, n_out, mono=mono,
                                              d_out=d_out[g0 * planes * pitch:], plane_pitch=pitch, stream=s,
                                              pcm_bytes=pcm_bytes)
            sts.append(st)
            g0 = g1
        with torch.cuda.stream(s):
            out = d_out[: k * planes * pitch].view(k, planes, pitch)[:, :, :n_out]
            if order != list(range(k)):
                back = np.empty(k, np.int64)
                back[np.asarray(order, np.int64)] = np.arange(k)
                out = out.index_select(0, torch.from_numpy(back).to(dev))
            if sts:
                both = torch.stack(sts)
                status["gather"] = torch.cat([both[:, :1].max(dim=0).values, both[:, 1:].sum(dim=0)]).to(torch.int32)
            else:
                status["gather"] = torch.zeros(4, dtype=torch.int32, device=dev)
        return out, status

    def gather_ranges_mel(self, d_pcm, fmt: int, sp: StreamParams, d_windows, nstreams: int, spec: MelSpec, d_tab, d_bands,
                          row_frames: int, mono: bool = False, d_out=None, frame_pitch: Optional[int] = None, stream=None,
                          pcm_bytes=None):
        """The windows of a decoded selection as mel (or power) spectrogram planes in one launch
        (bnflac_gather_ranges_mel): column t of row r of plane c of stream s is band r (bin r when
        spec.n_mels is 0) of STFT frame t of window s's channel c (mono: of the mean of the channels),
        frame t starting at sample spec.origin + t * spec.hop of the window; then zeros.  d_tab: a
        float32 device tensor of 2 * n_fft + n_weights values (window, twiddles, weights); d_bands: an
        int32 device tensor of n_mels + 1 pairs, or None when n_mels is 0 (mel_design makes both).
        The other arguments are gather_ranges_f32's, with row_frames and frame_pitch in row_samples'
        and plane_pitch's place.
        -> (float32[nstreams, planes, rows, row_frames], a view of d_out when one is passed; d_status
        int32[4]), on the device and not synchronised."""
        import torch
        dev = d_pcm.device
        s = stream if stream is not None else torch.cuda.current_stream()
        nbytes = d_pcm.numel() * d_pcm.element_size()
        planes = 1 if mono else sp.channels
        rows = spec.rows
        pitch = row_frames if frame_pitch is None else frame_pitch
        if pitch < row_frames:
            raise ValueError("frame_pitch is below row_frames")
        if d_tab.dtype != torch.float32 or not d_tab.is_contiguous() or d_tab.numel() != 2 * spec.n_fft + spec.n_weights:
            raise ValueError("d_tab is a contiguous float32 tensor of 2 * n_fft + n_weights values")
        if spec.n_mels and (d_bands is None or d_bands.element_size() != 4 or not d_bands.is_contiguous()
                            or d_bands.numel() != 2 * (spec.n_mels + 1)):
            raise ValueError("d_bands is a contiguous 32-bit tensor of n_mels + 1 pairs")
        with torch.cuda.stream(s):
            if d_out is None:
                d_out = torch.zeros(max(nstreams * planes * rows * pitch, 1), dtype=torch.float32, device=dev)
            d_status = torch.zeros(4, dtype=torch.int32, device=dev)
        if d_out.dtype != torch.float32 or not d_out.is_contiguous():
            raise ValueError("d_out is a contiguous float32 tensor")
        if nstreams and d_out.numel() < (nstreams * planes * rows - 1) * pitch + row_frames:
            raise ValueError("d_out is too small for nstreams * planes * rows rows")
        rc = self.L.bnflac_gather_ranges_mel(self.ctx, ctypes.c_void_p(d_pcm.data_ptr()),
                                             nbytes if pcm_bytes is None else min(pcm_bytes, nbytes), fmt,
                                             ctypes.byref(sp), ctypes.c_void_p(d_windows.data_ptr()), nstreams,
                                             ctypes.byref(spec), ctypes.c_void_p(d_tab.data_ptr()),
                                             ctypes.c_void_p(d_bands.data_ptr()) if spec.n_mels else None, row_frames, pitch,
                                             F32_MONO if mono else 0, ctypes.c_void_p(d_out.data_ptr()),
                                             ctypes.c_void_p(d_status.data_ptr()), self._stream(s))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())
        view = torch.as_strided(d_out.view(-1), (nstreams, planes, rows, row_frames),
                                (planes * rows * pitch, rows * pitch, pitch, 1))
        return view, d_status

    def decode_crops_mel(self, corpus: Corpus, crops, n_frames: int, mel, fmt: Optional[int] = None, mono: bool = False,
                         health: bool = False, stream=None, shared: bool = True):
        """Crops of an indexed corpus as mel (or power) spectrograms: n_frames STFT frames from frame
        t0 of a stream's own frame grid, with nothing read back.
        crops: [(stream, t0)]; mel: (MelSpec, tab, bands) as mel_design returns them, or with tab and
        bands already on the device (mel_to_device: upload them once and pass them to every call; host
        tables are uploaded again by each call, a blocking copy).  The requests, and the permutation
        when the crops have several origins, are uploaded from host memory per call as in decode_crops;
        apart from those copies nothing waits for the device.  mel_request
        turns every crop into a source window with the whole support of its frames, then
        select_windows[_shared] -> decode_parsed -> gather_ranges_mel; shared (the default) decodes a
        frame once for all the crops that overlap in it.  A crop past the stream's end is clipped by
        the selection and gives zeros there, as the whole stream in one window would.  One gather
        launch serves the crops that share an origin (all that do not start in front of the stream's
        sample 0); the crops are grouped by it.  health: as for decode_crops, over the source windows.
        -> (float32[k, planes, rows, n_frames] in request order, status: decode_crops' entries,
        "gather" the sum of the groups' status words with [0] their OR and [3] the bad bands)"""
        import torch
        sp = corpus.sp
        fmt = f32_layout(sp) if fmt is None else fmt
        if not md5_layout(fmt, sp):
            raise ValueError("the layout's bytes are not the samples: gather_ranges_mel cannot read it")
        if n_frames < 1:
            raise ValueError("n_frames must be at least 1")
        s = stream if stream is not None else torch.cuda.current_stream()
        dev = corpus.d_bytes.device
        spec, tab, bands = mel
        k = len(crops)
        planes = 1 if mono else sp.channels
        rows = spec.rows
        asked = [(int(t), ) + mel_request(spec, int(t0), n_frames) for t, t0 in crops]  # (stream, first, n, origin)
        order = sorted(range(k), key=lambda i: asked[i][3])
        requests = [asked[i][:3] for i in order]
        nsamples = max([r[2] for r in requests] + [1])
        d_pcm, d_win, _, pcm_bytes, status = self._decode_crop_selection(corpus, requests, nsamples, fmt, s, shared,
                                                                         health=health)
        pitch = (n_frames + 3) // 4 * 4  # every group's first row stays 16-byte aligned
        with torch.cuda.stream(s):
            _, d_tab, d_bands = mel_to_device(mel, dev)
            d_back = None
            if order != list(range(k)):  # the rows and the records back in request order: one upload
                back = np.empty(k, np.int64)
                back[np.asarray(order, np.int64)] = np.arange(k)
                d_back = torch.from_numpy(back).to(dev)
                if health:
                    status["windows_health"] = status["windows_health"].index_select(0, d_back)
            d_out = torch.zeros(max(k * planes * rows * pitch, 1), dtype=torch.float32, device=dev)
        sts, g0 = [], 0
        while g0 < k:
            g1 = g0
            while g1 < k and asked[order[g1]][3] == asked[order[g0]][3]:
                g1 += 1
            _, st = self.gather_ranges_mel(d_pcm, fmt, sp, d_win[g0 * WINDOW_BYTES:], g1 - g0,
                                           spec.with_origin(asked[order[g0]][3]), d_tab, d_bands, n_frames, mono=mono,
                                           d_out=d_out[g0 * planes * rows * pitch:], frame_pitch=pitch, stream=s,
                                           pcm_bytes=pcm_bytes)
            sts.append(st)
            g0 = g1
        with torch.cuda.stream(s):
            out = d_out[: k * planes * rows * pitch].view(k, planes, rows, pitch)[:, :, :, :n_frames]
            if d_back is not None:
                out = out.index_select(0, d_back)
            if sts:
                both = torch.stack(sts)
                status["gather"] = torch.cat([both[:, :1].max(dim=0).values, both[:, 1:3].sum(dim=0),
                                              both[:, 3:].max(dim=0).values]).to(torch.int32)
            else:
                status["gather"] = torch.zeros(4, dtype=torch.int32, device=dev)
        return out, status

    def crc_handoff(self, nframes: int) -> np.ndarray:
        """Debug: the CRC-16 hand-off of the last parse_frames call, [nframes, 8] uint32."""
        a = np.zeros(8 * nframes, np.uint32)
        if self.L.bnflac_debug_crc_handoff(self.ctx, a.ctypes.data_as(ctypes.c_void_p), nframes) != 0:
            raise RuntimeError(self.L.bnflac_last_error().decode())
        return a.reshape(nframes, 8)


class Reader:
    """Streaming PCM reader (include/bnflac.h part 3): Read(buffer, offset, count) like
    FLACDecoder.Read (FLACDecoder.cs:124-205), backed by GPU decode-ahead."""

    def __init__(self, data: bytes, out_format: int = OUT_FLACDECODER, window_frames: int = 0, device: int = 0):
        self.L = load()
        self._data = np.frombuffer(bytes(data), dtype=np.uint8)
        h = ctypes.c_void_p()
        rc = self.L.bnflac_reader_open(device, self._data.ctypes.data, self._data.size, out_format, window_frames,
                                       ctypes.byref(h))
        if rc != 0:
            raise RuntimeError(self.L.bnflac_reader_last_error().decode())
        self.h = h
        sp = StreamParams()
        tb, nf = ctypes.c_uint64(), ctypes.c_uint32()
        self.L.bnflac_reader_params(self.h, ctypes.byref(sp), ctypes.byref(tb), ctypes.byref(nf))
        self.stream_params, self.total_bytes, self.nframes = sp, int(tb.value), int(nf.value)

    def Read(self, buffer: bytearray, offset: int, count: int) -> int:
        if offset < 0 or count < 0 or offset + count > len(buffer):
            raise ValueError("offset/count outside the buffer")
        view = (ctypes.c_uint8 * len(buffer)).from_buffer(buffer)
        n = self.L.bnflac_reader_read(self.h, ctypes.addressof(view) + offset, count)
        if n < 0:
            raise RuntimeError(self.L.bnflac_reader_last_error().decode())
        return int(n)

    def ReadFileReader(self, buffer: bytearray, offset: int, count: int) -> int:
        """FLACFileReader.Read(buffer, offset, numBytes) semantics (bnflac_reader_read_filereader):
        copies may run past offset + count up to len(buffer); C# exceptions raise RuntimeError."""
        if offset < 0 or count < 0:
            raise ValueError("negative offset/count")
        view = (ctypes.c_uint8 * len(buffer)).from_buffer(buffer) if len(buffer) else None
        n = self.L.bnflac_reader_read_filereader(self.h, ctypes.addressof(view) if view is not None else None, offset,
                                                 count, len(buffer))
        if n < 0:
            raise RuntimeError(self.L.bnflac_reader_last_error().decode())
        return int(n)

    def filereader_read_all(self, buf_len: int, num_bytes: int = None):
        """Read(buf, 0, num_bytes) on a buf_len-byte buffer until 0, like
        oracle.filereader_readall -> (rc, bytes, message)."""
        num_bytes = buf_len if num_bytes is None else num_bytes
        out = bytearray()
        buf = bytearray(buf_len)
        try:
            while True:
                n = self.ReadFileReader(buf, 0, num_bytes)
                if n == 0:
                    return 0, bytes(out), ""
                out += buf[:n]
        except RuntimeError as e:
            return 1, bytes(out), str(e)

    def Seek(self, sample: int):
        """Next Read starts at this sample (per channel): FLACFileReader.Position."""
        if self.L.bnflac_reader_seek(self.h, sample) != 0:
            raise RuntimeError(self.L.bnflac_reader_last_error().decode())

    def read_all(self, chunk: int = 16384) -> bytes:
        out = bytearray()
        buf = bytearray(chunk)
        while True:
            n = self.Read(buf, 0, chunk)
            if n == 0:
                return bytes(out)
            out += buf[:n]

    def close(self):
        if getattr(self, "h", None):
            self.L.bnflac_reader_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def info_array(raw: np.ndarray) -> np.ndarray:
    """View a uint8 buffer of frame records as a structured array."""
    return np.frombuffer(np.ascontiguousarray(raw).tobytes(), dtype=FRAME_INFO_DTYPE)
