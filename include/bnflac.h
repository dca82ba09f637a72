/*
 * bnflac.h -- C ABI of libbnflac.so, the MI355X FLAC decoder behind BirdNest.Audio.
 *
 * Part 1: the libFLAC 1.2.1 stream-decoder entry points that BirdNest.Audio's P/Invoke
 * layer binds ([DllImport("LibFlac", CallingConvention = Cdecl)],
 * Library/LibFLACSharp/LibFLACSharp.cs:22).  Same names, argument meaning, return
 * conventions and callback order as libFLAC, so FLACDecoder / FLACFileReader /
 * OpenALDemo run unchanged when this library is loaded under the name "LibFlac"
 * (INTEGRATION.md).  Frame decode runs on the GPU; metadata and the libFLAC state
 * machine replay run on the host.
 *
 * Part 2: a batched, device-pointer API (bnflac_*) for callers that keep compressed
 * frames and PCM resident in HBM -- the path bench.py measures.  Whole .flac files in one
 * buffer go through it without the host reading anything back: bnflac_scan_streams (metadata)
 * -> bnflac_index_streams (frames) -> bnflac_parse_frames / bnflac_decode_parsed (PCM) ->
 * bnflac_md5_streams (verification), each asynchronous on the caller's HIP stream and chained by
 * device tables.  For one sample window per stream instead of whole streams, bnflac_select_ranges
 * goes between index and decode and bnflac_gather_ranges after the decode, or
 * bnflac_gather_ranges_f32 where the windows are wanted as float32 channel planes in [-1, 1).
 * For any crops of a batch that stays resident (several of one stream, none of most, in the
 * sampler's order), bnflac_select_windows takes bnflac_select_ranges' place over an index made once.
 * Where the crops overlap (sliding windows over whole recordings), bnflac_select_windows_shared takes
 * the same requests and selects every frame once, the windows pointing into one shared compact PCM.
 * After the decode of any of these selections, bnflac_window_health says per window how much of it lies
 * in frames that failed to decode or failed their CRC, and how much of the request the index lacks.
 * bnflac_index_streams ends a stream's frame chain at its first damaged frame.  For fixed-blocksize
 * streams bnflac_index_streams_resync takes its place and goes on at the next frame start that its
 * CRC-16 verifies, with placeholder records for the samples in between, so that only the damaged
 * frames are lost and every later call works on its tables unchanged.
 *
 * Only plain C types cross this boundary (no torch, no HIP types: a HIP stream is
 * passed as void*).
 */
#ifndef BNFLAC_H
#define BNFLAC_H

#include "FLAC_compat.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define BNFLAC_API __attribute__((visibility("default")))
#else
#define BNFLAC_API
#endif

/* ===================== Part 1: libFLAC-compatible stream decoder ===================== */

/* LibFLACSharp.cs:42-43 */
BNFLAC_API FLAC__StreamDecoder *FLAC__stream_decoder_new(void);
/* LibFLACSharp.cs:45-46 */
BNFLAC_API FLAC__bool FLAC__stream_decoder_finish(FLAC__StreamDecoder *decoder);
/* LibFLACSharp.cs:48-49 declares `bool` where libFLAC returns void; this export returns
 * true so FLACDecoder.cs:299-301's FLACCheck passes (SURVEY.md 8b hazard 1). */
BNFLAC_API FLAC__bool FLAC__stream_decoder_delete(FLAC__StreamDecoder *decoder);
/* LibFLACSharp.cs:51-52.  The C# write delegate is declared void (:205-206); its
 * return value is ignored for decoders initialised through init_file (hazard 2). */
BNFLAC_API int FLAC__stream_decoder_init_file(FLAC__StreamDecoder *decoder, const char *filename,
                                              FLAC__StreamDecoderWriteCallback write_callback,
                                              FLAC__StreamDecoderMetadataCallback metadata_callback,
                                              FLAC__StreamDecoderErrorCallback error_callback,
                                              void *client_data);
/* LibFLACSharp.cs:54-55 */
BNFLAC_API FLAC__bool FLAC__stream_decoder_process_single(FLAC__StreamDecoder *decoder);
/* LibFLACSharp.cs:57-58 */
BNFLAC_API FLAC__bool FLAC__stream_decoder_process_until_end_of_metadata(FLAC__StreamDecoder *decoder);
/* LibFLACSharp.cs:60-61 */
BNFLAC_API FLAC__bool FLAC__stream_decoder_process_until_end_of_stream(FLAC__StreamDecoder *decoder);
/* LibFLACSharp.cs:63-64 */
BNFLAC_API FLAC__bool FLAC__stream_decoder_seek_absolute(FLAC__StreamDecoder *decoder, FLAC__uint64 sample);
/* LibFLACSharp.cs:66-67 */
BNFLAC_API FLAC__bool FLAC__stream_decoder_get_decode_position(const FLAC__StreamDecoder *decoder,
                                                               FLAC__uint64 *position);
/* LibFLACSharp.cs:69-70 */
BNFLAC_API FLAC__uint64 FLAC__stream_decoder_get_total_samples(const FLAC__StreamDecoder *decoder);
/* LibFLACSharp.cs:72-79 */
BNFLAC_API unsigned FLAC__stream_decoder_get_channels(const FLAC__StreamDecoder *decoder);
BNFLAC_API unsigned FLAC__stream_decoder_get_bits_per_sample(const FLAC__StreamDecoder *decoder);
BNFLAC_API unsigned FLAC__stream_decoder_get_sample_rate(const FLAC__StreamDecoder *decoder);
/* LibFLACSharp.cs:81-82 */
BNFLAC_API FLAC__StreamDecoderState FLAC__stream_decoder_get_state(const FLAC__StreamDecoder *decoder);
/* LibFLACSharp.cs:84-85 (declared int in C#; libFLAC returns FLAC__bool) */
BNFLAC_API FLAC__bool FLAC__stream_decoder_reset(FLAC__StreamDecoder *decoder);
/* LibFLACSharp.cs:175-185 */
BNFLAC_API int FLAC__stream_decoder_init_stream(FLAC__StreamDecoder *decoder,
                                                FLAC__StreamDecoderReadCallback read_callback,
                                                FLAC__StreamDecoderSeekCallback seek_callback,
                                                FLAC__StreamDecoderTellCallback tell_callback,
                                                FLAC__StreamDecoderLengthCallback length_callback,
                                                FLAC__StreamDecoderEofCallback eof_callback,
                                                FLAC__StreamDecoderWriteCallback write_callback,
                                                FLAC__StreamDecoderMetadataCallback metadata_callback,
                                                FLAC__StreamDecoderErrorCallback error_callback,
                                                void *client_data);
/* libFLAC stream_decoder.h (not bound by LibFLACSharp.cs; BirdNest leaves MD5 checking
 * off).  Only while UNINITIALIZED; finish() then returns false when the MD5 of the
 * decoded PCM differs from STREAMINFO's non-zero md5sum.  A seek turns checking off. */
BNFLAC_API FLAC__bool FLAC__stream_decoder_set_md5_checking(FLAC__StreamDecoder *decoder, FLAC__bool value);
BNFLAC_API FLAC__bool FLAC__stream_decoder_get_md5_checking(const FLAC__StreamDecoder *decoder);

/* ========================= Part 2: batched device-pointer API ========================= */

typedef struct {
    int32_t has_stream_info;
    uint32_t min_blocksize, max_blocksize;
    uint32_t sample_rate, channels, bps;
    uint64_t total_samples;
} bnflac_stream_params;

/* Per-frame result record (128 bytes), device-resident. */
typedef struct {
    uint32_t status;        /* 0 ok, 1 libFLAC error (err), 2 truncated, 3 skipped */
    int32_t err;            /* FLAC__StreamDecoderErrorStatus, -1 none */
    uint64_t frame_off;
    uint64_t resume_bit;
    int32_t cached;
    uint32_t blocksize, sample_rate, channels, assignment, bps;
    uint32_t number_type, unparseable;
    uint64_t number;
    uint64_t out_sample;
    uint32_t crc8, crc16_calc, crc16_read, crc_ok;
    uint32_t sub_start[8];
    uint32_t flags;         /* bit 1: past out_bytes (status 3), bit 2: layout cannot carry it (status 3); the other
                               bits record the decode path (which kernel, hand-backs) and differ between paths */
    uint32_t reserved;      /* 0 */
} bnflac_frame_info;

enum {
    BNFLAC_OUT_PLANAR32 = 0,      /* int32, per frame channel-major (libFLAC write buffers) */
    BNFLAC_OUT_INTERLEAVED32 = 1, /* int32 [sample][channel] */
    BNFLAC_OUT_FLACDECODER = 2,   /* FLACDecoder.WriteCallback packing (FLACDecoder.cs:543-577) */
    BNFLAC_OUT_FILEREADER = 3     /* FLACFileReader packing (FLACFileReader.cs:220-237) */
};

typedef struct bnflac_ctx bnflac_ctx;

/* 0 on success, else a negative bnflac error code. */
BNFLAC_API int bnflac_ctx_create(int device, bnflac_ctx **out);
BNFLAC_API void bnflac_ctx_destroy(bnflac_ctx *ctx);
BNFLAC_API const char *bnflac_last_error(void);
BNFLAC_API int bnflac_device_count(void);

/* Find every frame-sync candidate (0xFF, then a byte with top 6 bits 111110) in
 * d_bytes[0, nbytes), in stream order.  d_bytes must be 4-byte aligned and its
 * allocation at least round_up(nbytes, 4) bytes.  *d_count (device) receives the total
 * (which may exceed cap; only cap offsets are written).  Asynchronous on hip_stream. */
BNFLAC_API int bnflac_index_frames(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes,
                                   uint64_t *d_offsets, uint32_t cap, uint32_t *d_count, void *hip_stream);

/* Frame chain resolution: the frames of a whole FLAC stream resident in
 * d_bytes (16-byte aligned, allocation >= round_up(nbytes, 16)), in stream order, without
 * decoding them.  Sync scan -> header, CRC-8 and subframe walk of every candidate ->
 * successor of each valid frame = the first later valid candidate at which the CRC-16 of
 * the bytes from the frame start is zero (the CRC-16 footer zeroes it; this is where
 * libFLAC's frame_sync_ finds the next frame in an intact stream) -> the chain from the
 * first valid candidate at or after first_offset (the byte after the metadata blocks).
 * Frames at or past STREAMINFO total_samples are dropped (frame_sync_'s end-of-stream
 * rule).  Writes d_frame_offsets, d_out_sample (running sample count; may be NULL) and,
 * when d_info != NULL, the parsed records ready for bnflac_decode_parsed.  *d_nframes
 * (device) = chain length (only cap entries are written).  A damaged stream ends the
 * chain at the damage; the libFLAC stream API handles resync, and so does
 * bnflac_index_streams_resync for the streams of a batch.  Synchronises hip_stream
 * once (candidate count); otherwise asynchronous. */
BNFLAC_API int bnflac_index_stream(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes, uint64_t first_offset,
                                   const bnflac_stream_params *sp, uint64_t *d_frame_offsets, uint64_t *d_out_sample,
                                   bnflac_frame_info *d_info, uint32_t cap, uint32_t *d_nframes, void *hip_stream);

/* One stream of a bnflac_index_streams batch.  The table is device-resident, one entry per
 * stream, ascending and non-overlapping. */
typedef struct {
    uint64_t begin, end;    /* the stream's bytes are d_bytes[begin, end); begin needs no alignment */
    uint64_t first_offset;  /* absolute offset in d_bytes of the byte after the metadata blocks */
    uint64_t total_samples; /* STREAMINFO total for the end-of-stream rule; 0 = unknown (no rule) */
} bnflac_stream_desc;

/* Status of one stream of bnflac_scan_streams: the first failure of its walk, in this order. */
enum {
    BNFLAC_SCAN_OK = 0,
    BNFLAC_SCAN_NO_MARKER = 1,       /* no "fLaC" at byte 0 or right after one ID3v2 tag */
    BNFLAC_SCAN_TRUNCATED = 2,       /* the tag, a block header, STREAMINFO or a block runs past the stream's end */
    BNFLAC_SCAN_NO_STREAMINFO = 3,   /* none before the last block, or one shorter than 34 bytes */
    BNFLAC_SCAN_TOO_MANY_BLOCKS = 4, /* no last-block flag within BNFLAC_SCAN_MAX_BLOCKS blocks */
    BNFLAC_SCAN_BAD_RANGE = 5        /* begin > end, end > nbytes, or begin below the previous entry's end */
};
enum { BNFLAC_SCAN_MAX_BLOCKS = 1024 };

/* Per-stream result record (64 bytes), device-resident. */
typedef struct {
    uint32_t status;      /* BNFLAC_SCAN_* */
    uint32_t flags;       /* bit 0 ID3v2 tag skipped, bit 1 STREAMINFO differs from the expected sp,
                             bit 2 md5sum all zero, bit 3 a SEEKTABLE block was met */
    uint32_t nblocks;     /* metadata block headers read */
    uint32_t id3_bytes;   /* bytes of the ID3v2 tag in front of the marker (0: none) */
    bnflac_stream_params sp;   /* offset 16; has_stream_info 1 when status is OK */
    uint32_t min_framesize, max_framesize;  /* offset 48 */
    uint64_t first_offset;     /* offset 56; absolute, as in bnflac_stream_desc */
} bnflac_stream_meta;

/* The metadata of every stream of a batch, read on the device: the first link of the chain
 * scan -> bnflac_index_streams -> parse / decode -> bnflac_md5_streams, none of which needs the
 * host to read anything back.  d_bytes as for bnflac_index_streams (16-byte aligned, allocation
 * >= round_up(nbytes, 16)).  d_streams is in/out: the caller fills begin and end of every entry
 * (ascending, non-overlapping; never written), the call writes first_offset and total_samples.
 * Per stream, over its bytes b[0, n), n = end - begin, the first failure deciding the status:
 *   a bad range (BAD_RANGE, nothing read); one optional ID3v2 tag at b[0] (libFLAC's
 *   skip_id3v2_tag_: 10 bytes + the 4 x 7-bit size; flags bit 0); "fLaC" exactly there
 *   (NO_MARKER); then blocks until the one with the last flag: header (TRUNCATED when cut;
 *   TOO_MANY_BLOCKS at BNFLAC_SCAN_MAX_BLOCKS), type 0 = STREAMINFO of at least 34 bytes
 *   (NO_STREAMINFO when shorter; a later one overwrites an earlier one; bytes past 34 skipped),
 *   type 3 sets flags bit 3, every type skipped by its length (TRUNCATED past the end).  No
 *   STREAMINFO met: NO_STREAMINFO.  Else OK, first_offset = begin + the bytes walked (== end: a
 *   stream of no frames).
 * libFLAC's find_metadata_ also searches junk byte by byte for the marker or a frame sync and
 * reports LOST_SYNC on the way; such streams are NO_MARKER here and belong to the stream API
 * (part 1).  Where this walk says OK, libFLAC reaches its first frame at the same offset with
 * the same STREAMINFO and no error event.
 * An OK stream is kept when expect is NULL or equals its STREAMINFO in min_blocksize,
 * max_blocksize, sample_rate, channels and bps: its descriptor gets first_offset and
 * STREAMINFO's total_samples, d_md5_expected (may be NULL; 16 bytes per stream) the md5sum, flags
 * bit 2 tells an all-zero one.  Every other stream is emptied: first_offset = end, total_samples
 * 0, md5sum zeros, so bnflac_index_streams yields no frame for it and bnflac_md5_streams verdict
 * 2, and stream positions in every later table stay those of the input.  An OK stream that
 * differs from expect has flags bit 1 and its own values (first_offset too) in its record; a
 * stream that is not OK has a record of zeros apart from status, flags, nblocks, id3_bytes and
 * first_offset = end.  d_meta may be NULL.
 * d_status (device, 4 words): [0] bit 0 some stream not OK, bit 1 some stream differs from
 * expect, bit 2 some BAD_RANGE; [1] streams kept; [2] streams not OK; [3] streams differing.
 * nstreams == 0 writes a zero status.  No byte at or past round_up(nbytes, 16) is read, and no
 * result depends on a byte outside [begin, end).  Asynchronous on hip_stream, no host
 * synchronisation. */
BNFLAC_API int bnflac_scan_streams(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes,
                                   bnflac_stream_desc *d_streams, uint32_t nstreams,
                                   const bnflac_stream_params *expect, bnflac_stream_meta *d_meta,
                                   uint8_t *d_md5_expected, uint32_t *d_status, void *hip_stream);

/* The same walk for one stream in host memory (begin 0, end nbytes, no expected parameters); no
 * GPU needed.  md5 (may be NULL) receives STREAMINFO's md5sum, zeros when meta->status is not
 * OK.  0, or -1 for a null meta or bytes. */
BNFLAC_API int bnflac_scan_stream_host(const uint8_t *bytes, uint64_t nbytes, bnflac_stream_meta *meta,
                                       uint8_t md5[16]);

/* bnflac_index_stream for many streams held in one buffer, in one call and with no host
 * synchronisation.  Stream s contributes exactly the frames bnflac_index_stream returns for
 * d_bytes[begin, end) alone with first_offset - begin and that stream's total_samples; sp is
 * shared by the batch (its total_samples is ignored).  The frames are concatenated in stream
 * order: stream s owns positions [d_stream_frames[s], d_stream_frames[s + 1]) of
 * d_frame_offsets (absolute offsets into d_bytes), d_out_sample (may be NULL: position in the
 * concatenated PCM, d_stream_samples[s] plus the stream's running sample count) and d_info
 * (may be NULL: the records with that out_sample, ready for one bnflac_decode_parsed over the
 * whole buffer).  d_stream_frames and d_stream_samples (may be NULL) have nstreams + 1
 * entries: the exclusive prefixes of the frames and samples kept per stream.  Only positions
 * below cap are written; d_stream_frames[nstreams] is the true total.
 * cand_cap bounds the sync candidates of the whole buffer (0: nbytes / 1024 + 4096) and sizes
 * the context's scratch, which a call may have to allocate.
 * d_status (device, 4 words): [0] flags -- bit 0 more candidates than cand_cap (outputs
 * unspecified, d_stream_frames all zero; retry with cand_cap = word 1), bit 1 more frames
 * than cap, bit 2 malformed table (begin > end, end > nbytes, first_offset outside
 * [begin, end], or out of order; outputs as for bit 0); [1] candidates found; [2] frames in
 * total; [3] 0.  nstreams == 0 or nbytes == 0 writes zeros.  A stream cut within the last
 * subframe's first byte of its last frame keeps that frame, with decode-class flags that
 * depend on the byte after the cut.  Asynchronous on hip_stream. */
BNFLAC_API int bnflac_index_streams(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes,
                                    const bnflac_stream_desc *d_streams, uint32_t nstreams,
                                    const bnflac_stream_params *sp, uint32_t cand_cap, uint64_t *d_frame_offsets,
                                    uint64_t *d_out_sample, bnflac_frame_info *d_info, uint32_t cap,
                                    uint32_t *d_stream_frames, uint64_t *d_stream_samples, uint32_t *d_status,
                                    void *hip_stream);

/* bnflac_frame_info.flags of a placeholder record of bnflac_index_streams_resync. */
#define BNFLAC_FRAME_GAP 0x800u

/* Per-stream result record of bnflac_index_streams_resync (32 bytes, 8-byte aligned), device-resident. */
typedef struct {
    uint32_t flags;       /* BNFLAC_RESYNC_* */
    uint32_t segments;    /* runs of CRC-linked frames kept: 0 for a stream without records, 1 for an intact one */
    uint32_t gap_frames;  /* placeholder records kept, saturating */
    uint32_t reserved;    /* 0 */
    uint64_t gap_samples; /* their samples: placeholders * blocksize */
    uint64_t base;        /* the stream position that is sample 0 of the stream's records */
} bnflac_resync_rec;
enum {
    BNFLAC_RESYNC_RESYNCED = 1,      /* the chain went on past at least one break */
    BNFLAC_RESYNC_CONTRADICTION = 2, /* it ended at a frame start whose number does not fit the samples before it */
    BNFLAC_RESYNC_HEAD = 4,          /* the first frame's number is no multiple of the blocksize or past the total: no records */
    BNFLAC_RESYNC_LEADING = 8        /* placeholders stand in front of the first frame */
};

/* bnflac_index_streams with resynchronisation, for fixed-blocksize streams: sp must have
 * has_stream_info and min_blocksize == max_blocksize = B >= 1, else the call returns a negative
 * value and launches nothing.  Arguments, tables, cand_cap, cap and the zero cases are
 * bnflac_index_streams'; d_resync (may be NULL) gets one record per stream.
 * With P = number * B for a header that codes a frame number, else the coded sample number, a
 * frame is linked to its CRC-16 successor (bnflac_index_streams' successor) when that frame's P
 * is this frame's P plus its blocksize.  The second condition is what this call adds to a link:
 * the CRC-16 of a run of zero bytes is zero, so a frame in front of zeroed frames closes at the
 * next surviving frame start too, and only the header numbers tell that the frames in between are
 * gone.  In an intact stream every successor is linked.
 * Where a frame has no linked successor -- there bnflac_index_streams ends the stream's chain, or
 * runs over a zeroed hole -- this call keeps that frame and goes on at the next frame start of the
 * stream that is verified: a valid candidate at or after first_offset, of blocksize B, with a
 * linked successor of its own, whose header number puts it on the stream's blocksize grid (below
 * total_samples when that is known).  With base = 0 when the stream's total_samples is known, else
 * the P of the stream's first frame (a stream of unknown length is rebased to its first frame, as
 * bnflac_index_streams does):
 *   - the first frame stands at P - base, with (P - base) / B placeholders in front of it
 *     (BNFLAC_RESYNC_LEADING).  When total_samples is known and P is no multiple of B or not below
 *     it, the stream gets no records (BNFLAC_RESYNC_HEAD);
 *   - inside a run of linked frames every frame stands at the end of the one before it, as in
 *     bnflac_index_streams;
 *   - after a break at stream position E (the end of the last frame kept), the next verified start
 *     stands at L = its P - base.  L < E, or L - E no multiple of B, ends the stream's chain before
 *     that start (BNFLAC_RESYNC_CONTRADICTION; later starts are not tried).  Otherwise (L - E) / B
 *     placeholders stand at E, E + B, ... and the chain goes on (BNFLAC_RESYNC_RESYNCED);
 *   - with total_samples known, the first frame at or past it ends the chain: it and everything
 *     after it are dropped, as in bnflac_index_streams, and nothing behind it sets a flag.  No
 *     placeholders follow the last frame kept.
 * A stream's records therefore tile [0, T), T = d_stream_samples[s + 1] - d_stream_samples[s], in
 * position order, which is all that bnflac_select_ranges, bnflac_select_windows[_shared],
 * bnflac_decode_parsed, both gathers, bnflac_md5_streams and bnflac_window_health rely on.  A
 * frame's record is the parsed record with out_sample = d_stream_samples[s] + its position.  A
 * placeholder is a record of zeros apart from status 1 with err 0 (lost sync), cached -1,
 * blocksize B, sample_rate, channels and bps of sp, number = position / B, out_sample,
 * sub_start[0] = 1 (so the decode zero-fills its range like that of any frame that failed after
 * its header) and flags = BNFLAC_FRAME_GAP; its frame_off and its d_frame_offsets entry are the
 * offset of the frame that follows the gap.  Placeholders are made for d_info ->
 * bnflac_decode_parsed: bnflac_parse_frames / bnflac_decode_frames over these offsets would parse
 * the following frame a second time in the placeholder's place.
 * Record counts are taken in 64 bits; the tables and the status hold min(count, 2^32 - 1), and only
 * positions below cap are written, however long a gap is.
 * d_status: [0] bits 0-2 as for bnflac_index_streams, bit 3 some stream has placeholders or
 * resynced, bit 4 some stream has CONTRADICTION or HEAD; [1] candidates found; [2] records in total;
 * [3] placeholders in total.
 * For a stream whose every successor is linked (its header numbers run on, as an encoder writes
 * them) and whose first frame has P == base, every output is byte for byte what
 * bnflac_index_streams writes.
 * Known limits: a frame between two damaged neighbours has no verified successor and is not
 * resumed at (libFLAC delivers it; here the chain goes on behind it, or ends, and
 * bnflac_window_health reports the rest as missing).  A contradiction ends the chain instead of
 * trying the next start.  Variable-blocksize streams are refused.  The CRC-16 hand-off of an
 * earlier bnflac_parse_frames is dropped, as by bnflac_index_streams.  Asynchronous on hip_stream,
 * no host synchronisation. */
BNFLAC_API int bnflac_index_streams_resync(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes,
                                           const bnflac_stream_desc *d_streams, uint32_t nstreams,
                                           const bnflac_stream_params *sp, uint32_t cand_cap, uint64_t *d_frame_offsets,
                                           uint64_t *d_out_sample, bnflac_frame_info *d_info, uint32_t cap,
                                           uint32_t *d_stream_frames, uint64_t *d_stream_samples,
                                           bnflac_resync_rec *d_resync, uint32_t *d_status, void *hip_stream);

/* One sync candidate as the indexer sees it after its first three steps (32 bytes). */
typedef struct {
    uint64_t offset;    /* of the 0xFF sync byte */
    uint64_t number;    /* the header's frame or sample number (0 unless valid) */
    int32_t succ;       /* the first later valid candidate of the stream at which this one's CRC-16 closes, -1 none
                           (as bnflac_index_streams takes it: the header numbers are not compared here) */
    int32_t stream;     /* the stream whose range holds it, -1 none */
    uint32_t blocksize; /* 0 unless valid */
    uint32_t flags;     /* bit 0 valid: parsed as a frame start inside its stream; bit 1 the number is a sample number */
} bnflac_index_cand;

/* One record position of bnflac_resync_plan_host (16 bytes). */
typedef struct {
    uint32_t cand;     /* the frame's candidate; for a placeholder, the frame that follows the gap */
    uint32_t gap;      /* 1 for a placeholder, else 0 */
    uint64_t position; /* first sample of the record inside its stream */
} bnflac_resync_slot;

/* The rule of bnflac_index_streams_resync as a plain walk over host tables (no GPU; the code of
 * csrc/bnf_resync.h that the kernels run).  The candidates of a stream are the entries with that
 * stream id, in table order; a succ that does not point forward inside the same stream counts as
 * none, as does one whose header numbers do not run on.  slots (cap entries; may be NULL) gets one entry per record position below cap,
 * stream_frames and stream_samples (nstreams + 1 entries each) the prefixes, resync (may be NULL)
 * the per-stream records, status the four words (bits 0 and 2 of word 0 are the device call's
 * own and stay 0; word 1 is ncand).  0, or a negative value with nothing written for B == 0, a
 * null table or output, or 2^30 or more entries. */
BNFLAC_API int bnflac_resync_plan_host(const bnflac_index_cand *cands, uint32_t ncand, const bnflac_stream_desc *streams,
                                       uint32_t nstreams, uint32_t B, bnflac_resync_slot *slots, uint32_t cap,
                                       uint32_t *stream_frames, uint64_t *stream_samples, bnflac_resync_rec *resync,
                                       uint32_t status[4]);

/* Debug: the candidate table of ctx's last bnflac_index_streams_resync call, synchronously: *ncand
 * candidates in all (0 when the table was malformed or cand_cap overflowed), min(*ncand, cap) of
 * them in out.  0, or -1 when the context holds none (no such call, or bnflac_index_streams has
 * reused the scratch since). */
BNFLAC_API int bnflac_debug_index_candidates(bnflac_ctx *ctx, bnflac_index_cand *out, uint32_t cap, uint32_t *ncand);

/* Decode nframes frames starting at d_frame_offsets (byte offsets into d_bytes).
 * Output position of each frame: d_out_sample[i] if non-NULL, else the header's
 * sample number (frame number x STREAMINFO blocksize for fixed-blocksize streams) minus
 * base_sample.  A frame is written only when its whole range lies in [0, out_bytes): with
 * stride = bnflac_out_stride (BNFLAC_OUT_FLACDECODER: by the frame's own channels) and
 * limit = out_bytes / stride, a frame of blocksize b at position p is written iff p <= limit
 * and b <= limit - p.  Positions are 64-bit and nothing in the rule wraps: a header number
 * below base_sample (the difference is taken modulo 2^64), or a table value whose byte range
 * does not fit (one near 2^64, one whose byte offset passes 2^64), is out of range like a frame
 * that ends past out_bytes: not one byte is written, status 3, flags bit 1.  The same rule
 * decides the zero-fill below.  d_out must be 4-byte aligned (the int32 layouts and the
 * 2-channel 16-bit layouts store whole dwords at multiples of 4 from d_out); any device
 * allocation is.  Which store path a frame takes (16-byte, 4-byte or byte stores, whole 64- or
 * 128-byte lines) follows its range's absolute address: the bytes never depend on it, the speed
 * does, and is best when d_out and the frames' starts are 128-byte aligned.
 * d_info receives one record per frame.  A frame whose status is not OK
 * (an error or truncation inside a subframe; libFLAC writes nothing for it) has its output
 * range zero-filled when its header parsed (sub_start[0] != 0), and is not written when the
 * header itself failed (no range).  A CRC-16 mismatch is status OK with crc_ok 0 and a
 * zero-filled frame, as libFLAC writes it.  Asynchronous on hip_stream. */
BNFLAC_API int bnflac_decode_frames(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes,
                                    const uint64_t *d_frame_offsets, uint32_t nframes,
                                    const bnflac_stream_params *sp, const uint64_t *d_out_sample,
                                    uint64_t base_sample, int out_format, uint8_t *d_out, uint64_t out_bytes,
                                    bnflac_frame_info *d_info, void *hip_stream);

/* The two phases of bnflac_decode_frames, for callers that time or overlap them:
 * parse = frame headers + subframe cursor walk (k_parse), decode = subframe decode,
 * decorrelation, packing and CRC-16 (k_decode).  decode must follow parse on the same
 * stream with the same arguments.  The parse also does part of the CRC-16 work of 2-channel
 * frames and hands it to the next bnflac_decode_parsed call on the same ctx with the same
 * d_bytes, nbytes, d_info and nframes (used once; bnflac_index_stream, bnflac_index_streams and bnflac_index_streams_resync drop it): the frame
 * bytes must not change between the two calls (bnflac_debug_set_crc_mode). */
BNFLAC_API int bnflac_parse_frames(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes,
                                   const uint64_t *d_frame_offsets, uint32_t nframes,
                                   const bnflac_stream_params *sp, const uint64_t *d_out_sample,
                                   uint64_t base_sample, bnflac_frame_info *d_info, void *hip_stream);
BNFLAC_API int bnflac_decode_parsed(bnflac_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes, uint32_t nframes,
                                    const bnflac_stream_params *sp, int out_format, uint8_t *d_out,
                                    uint64_t out_bytes, bnflac_frame_info *d_info, void *hip_stream);

/* Development switch: the kernels' ablation bits.  "Timing" bits skip parts of the kernels
 * (CRC-16, PCM stores, restore, Rice decode, the subframe walk): output is wrong while one is
 * set.  "Exact" bits are A/B switches between two implementations with identical PCM and
 * records (0x40 k_decode_st's running CRC-16 off, 0x800000 k_parse's block-by-block refill, ...).
 * The one list of the bits, with what each does and which kernels read it, is
 * birdnest/audio_amd/csrc/bnflac_launch.h (BNF_ABLATE_*).  Each kernel family receives only
 * the bits it defines; the launchers' own mode bits cannot be set from here.  Also read once
 * from BNFLAC_ABLATE in the environment.
 * 0x400 (k_decode_st not launched, k_decode<8> takes every stereo frame) also turns off the
 * split of k_decode<8> into two launches, as 0x100000 does: with no stereo fast-path frames
 * the split's two launches would leave most of them undecoded. */
BNFLAC_API void bnflac_debug_set_ablate(uint32_t flags);
/* Debug: 1 when the library was built with -DBNFLAC_CRC_FOLD_CHECK (never the shipped one):
 * k_decode_st's tail then computes the frame's CRC-16 both from the running remainder and from
 * the re-read, and bnflac_debug_stats slot 7 counts the lanes whose remainders differ. */
BNFLAC_API int bnflac_debug_crc_fold_check(void);
/* Development / test switch: parse kernel (-1 auto, 0 lane-per-frame k_parse, 1 wave-per-frame
 * k_parse_wave); both write identical records. */
BNFLAC_API void bnflac_debug_set_parse_wave(int mode);
/* Development / test switch: k_decode_sys, the systolic-restore decode of every frame class
 * (-1 auto: env BNFLAC_DECODE_SYS, else k_decode_sys for launches below 1024 subframe waves of
 * the lane kernels; 0 the lane kernels by class; 1 always); identical PCM and records. */
BNFLAC_API void bnflac_debug_set_decode_sys(int mode);
/* Development / test switch: who computes the CRC-16 hand-off bnflac_parse_frames passes to
 * bnflac_decode_parsed (-1 env BNFLAC_CRC_MODE, default 3; 0 none: the decode reads every frame
 * again; 1 k_parse's prefix: the lines before channel 1; 2 and its verdict over the span to
 * the next frame's offset; 3 the prefix, except for a 16-bit stream after a decode on the
 * device whose frames were a quarter or more LPC above order 8); identical PCM and records. */
BNFLAC_API void bnflac_debug_set_crc_mode(int mode);
/* Debug: the hand-off of ctx's last bnflac_parse_frames call (8 words per frame: prefix
 * remainder r0, r1 | parity << 31, its lines + 1, frame_off low word; span to the next
 * offset, verdict over it, frame_off low word, 0), synchronously.  0, or -1 when none. */
BNFLAC_API int bnflac_debug_crc_handoff(bnflac_ctx *ctx, uint32_t *out, uint32_t nframes);
/* Debug: how many decodes of this process took the W16 / W32 classes through one small
 * segment grid (k_decode_seg: the previous decode order on the device had neither class)
 * instead of the two full-size side grids. */
BNFLAC_API uint64_t bnflac_debug_decode_seg_launches(void);
/* Debug: the route of the process's last decode launch and last parse launch (bnflac_decode_parsed /
 * bnflac_parse_frames, or the two halves of bnflac_decode_frames), whatever the context or device.
 * A decode picks its kernels and streams from the class counts the previous decode on the device
 * left in host memory ("history"), so a test that primes a history reads here that it got the
 * route it meant.  out12 receives 12 words:
 *   [0]     the decode: 1 k_decode_sys (+ k_decode_list); otherwise exactly one of 2 side grids forked
 *           before k_decode_st, 4 forked after it, 8 serial (the W16 / W32 grids on the caller's
 *           stream), 16 k_decode_seg instead of them; plus 32 k_decode<8> as two launches, 64
 *           k_decode_sw ran first, 128 the history words were read
 *   [1..4]  the history words it read (with bit 128): W16 frames, W32 frames, all frames, class-1
 *           frames of the previous decode order; 0xFFFFFFFF each before the first decode on the device
 *   [5]     decode launches so far
 *   [6]     the parse: 1 k_parse_wave ran (it produces no hand-off), 2 the history was consulted
 *           for the hand-off mode
 *   [7]     the CRC-16 hand-off mode launched: 0 none, 1 the prefix, 2 and the verdict
 *   [8]     parse launches so far
 *   [9..11] the history words the parse read (with bit 2 of [6]): W16, W32, all frames
 * Written with relaxed host atomics by the launchers: meaningful while one thread launches. */
BNFLAC_API void bnflac_debug_last_route(uint32_t *out12);
/* Debug: k_parse_wave's counters, collected while BNFLAC_PW_STATS is set in the environment
 * (passes, splice rounds, serial fallbacks, partitions, frames, scan / window-wait / splice
 * wave-cycles).  out8 holds 8 values; reset != 0 clears them.  0 or -1. */
BNFLAC_API int bnflac_debug_parse_wave_stats(uint64_t *out8, int reset);
/* Debug: k_decode event counters collected while ablate bit 0x100 is set: [0..5] fused
 * chunks, generic chunks, DMA landing waits, slow Rice codewords, refills, waves (wave-level
 * events); [6] k_decode_st frames whose tail continued the running CRC-16 of channel 1; [7]
 * see bnflac_debug_crc_fold_check; [8..12] shader-clock cycles summed over waves in setup, chunk decode, refill,
 * pack, tail.  out16 holds 16 values.  Synchronous; reset != 0 clears them. */
BNFLAC_API int bnflac_debug_stats(uint64_t *out16, int reset);

/* Bytes of one sample frame (all channels of one sample index) in out_format. */
BNFLAC_API uint32_t bnflac_out_stride(int out_format, const bnflac_stream_params *sp);

/* Host helper: STREAMINFO md5sum of nsamples interleaved int32 sample frames (host
 * memory, e.g. a BNFLAC_OUT_INTERLEAVED32 result copied back), hashed as libFLAC does:
 * each sample as (bps + 7) / 8 little-endian bytes.  0 on success. */
BNFLAC_API int bnflac_md5_interleaved32(const int32_t *pcm, uint64_t nsamples, uint32_t channels, uint32_t bps,
                                        uint8_t out_md5[16]);

/* Bytes per sample of the STREAMINFO MD5 message when out_format's bytes can be hashed by
 * bnflac_md5_streams for sp, else 0 (PLANAR32; FLACDECODER unless 16-bit with 1-2 channels;
 * FILEREADER unless 16- or 24-bit; bps outside 4..32).  Host only, no GPU needed. */
BNFLAC_API uint32_t bnflac_md5_layout(int out_format, const bnflac_stream_params *sp);

/* STREAMINFO md5sum of every stream of a decoded batch, on the device.  Stream s is the sample
 * frames [d_stream_samples[s], d_stream_samples[s + 1]) of d_pcm in out_format (nstreams + 1
 * entries: what bnflac_index_streams writes; for one stream, {0, total}).  d_pcm 16-byte aligned,
 * its allocation at least round_up(pcm_bytes, 4) bytes.
 * d_md5: 16 bytes per stream.  d_expected (may be NULL): 16 bytes per stream, STREAMINFO's sums.
 * d_verdict (may be NULL), one word per stream: 0 equal, 1 differs, 2 not checked (d_expected NULL
 * or all zero: libFLAC's "not computed"), 3 range descending or past pcm_bytes (sum written as
 * zeros).  d_status, 4 words: [0] bit 0 = some stream had verdict 3, [1] streams equal,
 * [2] streams differing, [3] streams not checked.  Hashes whatever the decode left in the range
 * (a CRC-failed frame's zeros, as libFLAC does).  nstreams == 0 writes a zero status.
 * Asynchronous on hip_stream, no host synchronisation. */
BNFLAC_API int bnflac_md5_streams(bnflac_ctx *ctx, const uint8_t *d_pcm, uint64_t pcm_bytes, int out_format,
                                  const bnflac_stream_params *sp, const uint64_t *d_stream_samples,
                                  uint32_t nstreams, const uint8_t *d_expected, uint8_t *d_md5,
                                  uint32_t *d_verdict, uint32_t *d_status, void *hip_stream);

/* One stream's window of bnflac_select_ranges, in the stream's own samples. */
typedef struct {
    uint64_t first_sample, nsamples;
} bnflac_sample_range;

/* Per-stream result record of bnflac_select_ranges (32 bytes), device-resident. */
typedef struct {
    uint64_t pcm_first;     /* sample frame of the compact PCM at which the window starts (= d_sel_samples[s] + skip) */
    uint64_t nsamples;      /* samples of the window after clipping at the stream's end */
    uint32_t skip;          /* samples of the first selected frame in front of the window (< its blocksize) */
    uint32_t first_frame;   /* position in the index's tables of the first selected frame (d_stream_frames[s] when none) */
    uint32_t nframes;       /* frames selected */
    uint32_t flags;         /* bit 0 clipped by the stream's end, bit 1 empty */
} bnflac_window;

/* Cut the tables of bnflac_index_streams down to the frames that one sample window per stream
 * needs, on the device: index -> bnflac_select_ranges -> bnflac_decode_parsed(nframes = sel_cap)
 * -> bnflac_gather_ranges decodes "samples [a, a + n) of every stream" without decoding the rest
 * and without the host reading anything back.  d_frame_offsets (may be NULL with d_sel_offsets),
 * d_info, cap, d_stream_frames and d_stream_samples are the index call's outputs and its cap;
 * d_info and d_sel_info are 16-byte aligned.
 * Per stream s, with T = d_stream_samples[s + 1] - d_stream_samples[s], and for every frame i of
 * [d_stream_frames[s], d_stream_frames[s + 1]) its local start L_i = d_info[i].out_sample -
 * d_stream_samples[s] and its blocksize b_i:
 *   lo = min(first_sample, T), hi = min(lo + nsamples, T), the sum saturating (nsamples =
 *   UINT64_MAX: to the end).  hi == lo: the window is empty (flags bit 1, nframes 0, skip 0,
 *   nsamples 0, pcm_first = d_sel_samples[s]).  Else the frames with L_i < hi and L_i + b_i > lo
 *   are selected, a contiguous run [a, b) (a frame that only touches the window, L_i == hi or
 *   L_i + b_i == lo, is not): first_frame = a, nframes = b - a, skip = lo - L_a, nsamples =
 *   hi - lo.  flags bit 0 when first_sample + nsamples (saturating) exceeds T.
 * The selected records are copied byte for byte apart from out_sample, which becomes
 * d_sel_samples[s] + (L_i - L_a): the selection decodes into a compact PCM in which stream s owns
 * the sample frames [d_sel_samples[s], d_sel_samples[s + 1]), the frame-aligned hull of its
 * window.  d_sel_offsets (may be NULL) gets the matching d_frame_offsets entries.  d_sel_frames
 * and d_sel_samples (nstreams + 1 entries each) are the exclusive prefixes of the frames and
 * samples selected per stream; their last entry is the true total.  Positions [total, sel_cap) of
 * d_sel_info are filler records: zeros apart from status 3 (skipped) and err -1, d_sel_offsets 0;
 * every decode kernel leaves a record alone whose status is not OK, so bnflac_decode_parsed can
 * run over sel_cap records without the count being read back.
 * d_status (device, 4 words): [0] bit 0 more frames selected than sel_cap (the records below
 * sel_cap are written, the tables are the true prefixes, a stream whose frames all lie below
 * sel_cap is complete), bit 1 the tables are unusable (d_stream_frames[nstreams] > cap: the index
 * overflowed, or d_stream_frames / d_stream_samples descend): nothing is selected, both prefix
 * tables are zero, every window is empty and every record below sel_cap is filler; [1] frames
 * selected; [2] streams with a non-empty window; [3] streams clipped.  nstreams == 0 writes a
 * zero status and fills d_sel_info.  A failed index call (d_stream_frames all zero) selects nothing.
 * Nothing at or past position cap of the index's tables is read, nothing at or past sel_cap is
 * written, and no loop is bounded by a table's contents: over out_sample values the index did not
 * write, the searches still end inside the stream's frames, with some window.  Asynchronous on
 * hip_stream, no host synchronisation; the only allocation is a scratch kept in ctx that grows
 * with nstreams. */
BNFLAC_API int bnflac_select_ranges(bnflac_ctx *ctx, const uint64_t *d_frame_offsets, const bnflac_frame_info *d_info,
                                    uint32_t cap, const uint32_t *d_stream_frames, const uint64_t *d_stream_samples,
                                    uint32_t nstreams, const bnflac_sample_range *d_ranges, uint64_t *d_sel_offsets,
                                    bnflac_frame_info *d_sel_info, uint32_t sel_cap, uint32_t *d_sel_frames,
                                    uint64_t *d_sel_samples, bnflac_window *d_windows, uint32_t *d_status,
                                    void *hip_stream);

/* The same selection over tables in host memory, with the same results; no GPU needed.  0, or -1
 * for a null argument. */
BNFLAC_API int bnflac_select_ranges_host(const bnflac_frame_info *info, uint32_t cap, const uint32_t *stream_frames,
                                         const uint64_t *stream_samples, uint32_t nstreams,
                                         const bnflac_sample_range *ranges, bnflac_frame_info *sel_info, uint32_t sel_cap,
                                         uint32_t *sel_frames, uint64_t *sel_samples, bnflac_window *windows,
                                         uint32_t status[4]);

/* One crop of bnflac_select_windows: a sample window of stream `stream` of the index's tables. */
typedef struct {
    uint64_t stream;                 /* position in the index's tables; >= nstreams: no such stream */
    uint64_t first_sample, nsamples; /* as bnflac_sample_range */
} bnflac_window_request;             /* 24 bytes, 8-byte aligned: 3 64-bit words, a [nwindows, 3] int64 tensor */

enum { BNFLAC_WIN_NO_STREAM = 4 };   /* bnflac_window.flags bit 2, only written by bnflac_select_windows */

/* bnflac_select_ranges with the window as its unit: any crops of an indexed batch, in the order
 * they are asked for.  Each of the nwindows requests names the stream it wants a piece of; any
 * number may name the same stream, in any order, and a stream nobody names costs nothing.  The
 * tables (d_frame_offsets, d_info, cap, d_stream_frames, d_stream_samples, nstreams) are one earlier
 * bnflac_index_streams call's and are only read, so one index serves any number of calls: per batch
 * the chain is bnflac_select_windows -> bnflac_decode_parsed(nframes = sel_cap) ->
 * bnflac_gather_ranges / bnflac_gather_ranges_f32 with nstreams = nwindows.
 * Per window w, with t = d_requests[w].stream: t >= nstreams gives an empty window with flags bit 1
 * and bit 2 (first_frame 0, nframes 0, skip 0, nsamples 0), and no table entry is read for it.
 * Otherwise the window is bnflac_select_ranges' rule over stream t's slice of the tables with
 * (first_sample, nsamples): the same lo and hi, saturating sum, clipping flag, "a frame that only
 * touches is not selected", and skip.
 * The outputs are per window, in request order.  d_sel_frames and d_sel_samples (nwindows + 1
 * entries each) are the exclusive prefixes of the frames and hull samples selected per window;
 * window w owns the sample frames [d_sel_samples[w], d_sel_samples[w + 1]) of the compact PCM,
 * pcm_first = d_sel_samples[w] + skip, and its records are the selected records copied byte for
 * byte apart from out_sample = d_sel_samples[w] + (L_i - L_a).  Two windows on one stream each get
 * their own copy of the frames they need: a frame both need is copied and decoded twice, nothing
 * is deduplicated.  Positions [total, sel_cap) are filler records, as for bnflac_select_ranges.
 * So the frame total is not bounded by cap.  Frames are counted in 64 bits, and d_sel_frames and
 * status word 1 hold min(prefix, UINT32_MAX); a saturated total exceeds every sel_cap (bit 0), and
 * the records below sel_cap are exactly right, since they only depend on prefix entries <= their
 * position.  Sample prefixes are modulo 2^64, as all sample arithmetic here.
 * d_status (device, 4 words): [0] bit 0 more frames selected than sel_cap, bit 1 unusable tables,
 * bit 2 some request names no stream; [1] frames selected (saturating); [2] windows that are not
 * empty; [3] windows clipped.  Unusable is judged only on the slices some request names
 * (d_stream_frames[t] <= d_stream_frames[t + 1] <= cap, d_stream_samples[t] <= d_stream_samples[t + 1]):
 * a bad slice nobody names is not read and is no error.  If a named slice is bad, nothing is
 * selected, as for bnflac_select_ranges: both prefix tables are zero, every record below sel_cap is
 * filler, words 1-3 are 0, and every window is empty with first_frame = d_stream_frames[t] (a
 * request without a stream keeps first_frame 0 and bit 2 of its flags).  Bit 2 of word 0 is
 * reported whether or not bit 1 is.  nwindows == 0 writes a zero status, the single prefix entries
 * and the filler; nstreams == 0 with nwindows > 0 is legal, every window then names no stream.
 * For nwindows == nstreams and d_requests[s] = {s, d_ranges[s]}, every output is byte-identical to
 * bnflac_select_ranges'.
 * A negative return (nothing launched, nothing written): the null-pointer, alignment and
 * d_sel_offsets-without-d_frame_offsets rules of bnflac_select_ranges, d_requests not 8-byte
 * aligned, nwindows >= 2^30.
 * No grid, loop bound or scratch size depends on nstreams or on a table's contents.  Nothing at or
 * past position cap of the index's tables is read; nothing at or past sel_cap, nwindows (d_windows)
 * or nwindows + 1 (the prefix tables) is written.  Asynchronous on hip_stream, no host
 * synchronisation, on ctx's device; the only allocation is bnflac_select_ranges' scratch in ctx,
 * which grows with nwindows (8 bytes per window) and never shrinks. */
BNFLAC_API int bnflac_select_windows(bnflac_ctx *ctx, const uint64_t *d_frame_offsets, const bnflac_frame_info *d_info,
                                     uint32_t cap, const uint32_t *d_stream_frames, const uint64_t *d_stream_samples,
                                     uint32_t nstreams, const bnflac_window_request *d_requests, uint32_t nwindows,
                                     uint64_t *d_sel_offsets, bnflac_frame_info *d_sel_info, uint32_t sel_cap,
                                     uint32_t *d_sel_frames, uint64_t *d_sel_samples, bnflac_window *d_windows,
                                     uint32_t *d_status, void *hip_stream);

/* The same selection over tables in host memory, with the same results; no GPU needed.  0, or -1
 * for a null argument or nwindows >= 2^30. */
BNFLAC_API int bnflac_select_windows_host(const bnflac_frame_info *info, uint32_t cap, const uint32_t *stream_frames,
                                          const uint64_t *stream_samples, uint32_t nstreams,
                                          const bnflac_window_request *requests, uint32_t nwindows,
                                          bnflac_frame_info *sel_info, uint32_t sel_cap, uint32_t *sel_frames,
                                          uint64_t *sel_samples, bnflac_window *windows, uint32_t status[4]);

/* bnflac_select_windows for windows that overlap: the union of the frames the windows need, each
 * selected, copied and decoded once, and window records that point into that shared compact PCM.
 * With a window W and a hop H < W over a stream, bnflac_select_windows selects every frame about
 * W / H times; this call selects it once.  The inputs are bnflac_select_windows', and so is the rule
 * per window w: its run [a_w, a_w + n_w) of index positions, skip_w, nsamples_w and flags_w (no
 * stream, clipping, "a frame that only touches is not selected"), and unusable slices are judged only
 * where a request names them.  The chain is bnflac_select_windows_shared ->
 * bnflac_decode_parsed(nframes = sel_cap) -> bnflac_gather_ranges / bnflac_gather_ranges_f32 with
 * nstreams = nwindows; the gathers take any window table, and two windows may read the same PCM.
 * If some named slice is unusable, the outcome is bnflac_select_windows': nothing is selected, every
 * window is empty with first_frame = d_stream_frames[t] (0 and flags bit 2 without a stream), every
 * record below sel_cap is filler, the totals and status words 1-3 are 0, bit 1 of word 0 is set and
 * bit 2 is still reported.
 * Otherwise let M be the index positions in the union over w of [a_w, a_w + n_w), and for i in M, in
 * ascending position order, rank_i = the members of M below i, pos_i = the sum of their blocksizes
 * (modulo 2^64), F = |M| and S = the sum of the blocksizes over M.
 *   d_sel_info[rank_i]: d_info[i] byte for byte apart from out_sample = pos_i, written only where
 *     rank_i < sel_cap; d_sel_offsets[rank_i] (may be NULL) = d_frame_offsets[i].  Positions
 *     [F, sel_cap) are the filler records of bnflac_select_ranges, d_sel_offsets 0.
 *   d_windows[w] (nwindows records): for a window that is not empty pcm_first = pos_{a_w} + skip_w;
 *     nsamples, skip, first_frame = a_w, nframes = n_w and flags as bnflac_select_windows writes them.
 *     An empty window is as there, with pcm_first = 0.
 *   d_win_sel_first[w] (uint32, nwindows entries, may be NULL): rank_{a_w} for a window that is not
 *     empty, else 0.  Over an index's tables window w's records are [that, that + nframes) of
 *     d_sel_info: their status / crc_ok can be read there after the decode.
 *   d_sel_totals (uint64[2], 8-byte aligned): {F, S}; S is the sample frames of the shared compact PCM.
 *   d_status (4 words): [0] bit 0 F > sel_cap (the records below sel_cap are exactly right, every
 *     window record is written from the true positions, a window whose records all lie below sel_cap
 *     is complete), bit 1 unusable tables, bit 2 some request names no stream; [1] F (at most cap:
 *     nothing saturates); [2] windows that are not empty; [3] windows clipped.
 * nwindows == 0 writes a zero status, zero totals and the filler.
 * Over tables bnflac_index_streams wrote, the frames of a stream tile it, so a window's run is
 * contiguous in rank and in pos with the spacing out_sample had: window w read through d_windows[w]
 * is byte-identical to what the bnflac_select_windows chain yields for it.  Over any other contents
 * the call returns some windows and never faults; no trip count is a table value.
 * A negative return (nothing launched, nothing written): the refusals of bnflac_select_windows, and
 * d_sel_totals not 8-byte aligned.
 * Grids, loop bounds and scratch sizes depend on cap, nwindows and sel_cap only (a workgroup past the
 * last position any window covers leaves at once).  Nothing at or past position cap of the index's
 * tables is read, and d_info only at positions of M; nothing at or past sel_cap (records, offsets),
 * nwindows (d_windows, d_win_sel_first) or entry 2 of the totals is written.  Asynchronous on
 * hip_stream, no host synchronisation, on ctx's device; the only allocation is bnflac_select_ranges'
 * scratch in ctx, which never shrinks: 16 bytes per position of [0, cap] plus 16 per 1,024 positions,
 * nothing per window (the window records are completed in place).  With bnflac_index_streams' cap a
 * bound from the buffer's size, that is the price of the call: pass the index's frame count (known
 * after one read-back) as cap where the memory matters. */
BNFLAC_API int bnflac_select_windows_shared(bnflac_ctx *ctx, const uint64_t *d_frame_offsets,
                                            const bnflac_frame_info *d_info, uint32_t cap,
                                            const uint32_t *d_stream_frames, const uint64_t *d_stream_samples,
                                            uint32_t nstreams, const bnflac_window_request *d_requests, uint32_t nwindows,
                                            uint64_t *d_sel_offsets, bnflac_frame_info *d_sel_info, uint32_t sel_cap,
                                            bnflac_window *d_windows, uint32_t *d_win_sel_first, uint64_t *d_sel_totals,
                                            uint32_t *d_status, void *hip_stream);

/* The same selection over tables in host memory, with the same results; no GPU needed.  0, or -1
 * for a null argument, nwindows >= 2^30 or no memory for cap + 1 marks. */
BNFLAC_API int bnflac_select_windows_shared_host(const bnflac_frame_info *info, uint32_t cap,
                                                 const uint32_t *stream_frames, const uint64_t *stream_samples,
                                                 uint32_t nstreams, const bnflac_window_request *requests,
                                                 uint32_t nwindows, bnflac_frame_info *sel_info, uint32_t sel_cap,
                                                 bnflac_window *windows, uint32_t *win_sel_first, uint64_t sel_totals[2],
                                                 uint32_t status[4]);

/* Per-window result record of bnflac_window_health (32 bytes, 8-byte aligned), device-resident. */
typedef struct {
    uint32_t flags;        /* BNFLAC_HEALTH_* */
    uint32_t bad_frames;   /* records of the window's run, below sel_cap, that are not good */
    uint32_t crc_frames;   /* of those: status OK with crc_ok 0 */
    uint32_t reserved;     /* 0 */
    uint64_t bad_samples;  /* sample frames of the window that lie in records that are not good */
    uint64_t missing;      /* sample frames the request asked for that STREAMINFO promises and the index lacks */
} bnflac_window_health_rec;

enum { BNFLAC_HEALTH_DAMAGED = 1, BNFLAC_HEALTH_SHORT = 2, BNFLAC_HEALTH_UNKNOWN = 4,
       BNFLAC_HEALTH_EMPTY = 8, BNFLAC_HEALTH_NO_STREAM = 16 };

/* Which windows of a decoded selection hold damaged or missing audio.  A frame that fails to decode
 * or fails its CRC-16 leaves zeros in the compact PCM, and a stream the index cut short at its damage
 * gives clipped or empty windows; neither shows in the rows, nor in the select and gather status
 * words, which describe the tables.  This call reduces the completed records per window, after
 * bnflac_decode_parsed on the same stream, with nothing read back.
 * d_sel_info, sel_cap: the selection's records after the decode.  d_windows: its window table.
 * d_first[w]: the position in d_sel_info of window w's first record -- d_sel_frames for
 * bnflac_select_ranges and bnflac_select_windows (only its first nwindows entries are read),
 * d_win_sel_first for bnflac_select_windows_shared.  d_requests, d_streams, d_stream_samples: all NULL
 * (missing is then 0 everywhere, SHORT and NO_STREAM are never set), or the requests the selection was
 * made from, the descriptor table bnflac_scan_streams completed and the index's d_stream_samples and
 * nstreams (a bnflac_select_ranges caller builds {s, d_ranges[s]} as d_requests).
 * A record is good iff status == 0 && crc_ok != 0, else bad; a bad record with status == 0 is a crc
 * record.  Per window w, with W = d_windows[w], f = d_first[w], n = W.nframes:
 *   the run R = [min(f, sel_cap), min(f + n, sel_cap)), the sum taken in 64 bits;
 *   bad_frames, crc_frames = the bad and the crc records of R; A = the sum of blocksize over R, B =
 *   the sum over the bad records of R (modulo 2^64);
 *   head = W.skip if n > 0, f < sel_cap and record f is bad, else 0;
 *   tail = A - W.skip - W.nsamples (modulo 2^64) if n > 0, f + n <= sel_cap and record f + n - 1 is
 *   bad, else 0;  bad_samples = B - head - tail (modulo 2^64).
 *   flags: UNKNOWN iff n > 0 and f + n > sel_cap (some of the window's records were not provided: what
 *   lies below sel_cap is counted, no tail is taken); EMPTY = W.flags bit 1; DAMAGED iff bad_frames != 0.
 * Over tables a selection wrote from an index and a decode completed, a stream's frames tile it, and
 * bad_samples is exactly the number of the window's sample frames that lie inside bad frames (a window
 * of one bad frame: W.nsamples).  Only status, crc_ok and blocksize of a record are read.
 * With the request tables, t = d_requests[w].stream:  t >= nstreams sets NO_STREAM, missing is 0 and no
 * table entry is read for t.  Else total = d_streams[t].total_samples, T = d_stream_samples[t + 1] -
 * d_stream_samples[t], lo = first_sample, hi = first_sample + nsamples (saturating), promised =
 * min(hi, total) - min(lo, total), have = min(hi, T) - min(lo, T), and missing = promised - have if
 * total > T and promised > have, else 0; SHORT iff missing != 0.  total == 0 (unknown, or the stream
 * was emptied by the scan, whose status says why) means nothing is missing.  A crop clipped by the
 * stream's true end is not SHORT; one that reaches into what damage cut off is, also when its window is
 * empty, which the row alone can never show.
 * d_status (device, 4 words): [0] bit 0 some window is DAMAGED, bit 1 some is SHORT, bit 2 some is
 * UNKNOWN; [1] windows DAMAGED; [2] windows SHORT; [3] windows UNKNOWN.  nwindows == 0 writes a zero
 * status.
 * A negative return (nothing launched, nothing written, the cause in bnflac_last_error()): a null ctx,
 * d_sel_info, d_windows, d_first, d_health or d_status; only some of the three request tables given;
 * d_sel_info not 16-byte aligned; d_windows, d_requests, d_streams, d_stream_samples or d_health not
 * 8-byte aligned; d_first or d_status not 4-byte aligned; nwindows >= 2^30.
 * Nothing at or past sel_cap of the records is read, nothing at or past nwindows of the window, first
 * and request tables, nothing of d_streams or d_stream_samples for a t >= nstreams; nothing at or past
 * nwindows records of d_health or 4 words of d_status is written.  Over any table contents the call
 * returns some values and never faults: no grid, loop bound or scratch size is a table value, they
 * depend on sel_cap and nwindows only (prefixes over the record positions, then one lane per window).
 * Asynchronous on hip_stream, no host synchronisation, on ctx's device; the only allocation is
 * bnflac_select_ranges' scratch in ctx, which never shrinks: 24 bytes per position of [0, sel_cap) plus
 * 24 per 1,024 positions, nothing per window. */
BNFLAC_API int bnflac_window_health(bnflac_ctx *ctx, const bnflac_frame_info *d_sel_info, uint32_t sel_cap,
                                    const bnflac_window *d_windows, const uint32_t *d_first, uint32_t nwindows,
                                    const bnflac_window_request *d_requests, const bnflac_stream_desc *d_streams,
                                    const uint64_t *d_stream_samples, uint32_t nstreams,
                                    bnflac_window_health_rec *d_health, uint32_t *d_status, void *hip_stream);

/* The same records and status over tables in host memory, by the same code (csrc/bnf_health.h); no GPU
 * needed.  Refuses what the device call refuses apart from ctx and pointer alignment.  0, or -1 for
 * such an argument or no memory for sel_cap + 1 prefixes. */
BNFLAC_API int bnflac_window_health_host(const bnflac_frame_info *sel_info, uint32_t sel_cap, const bnflac_window *windows,
                                         const uint32_t *first, uint32_t nwindows, const bnflac_window_request *requests,
                                         const bnflac_stream_desc *streams, const uint64_t *stream_samples,
                                         uint32_t nstreams, bnflac_window_health_rec *health, uint32_t status[4]);

/* The windows of a decoded selection as rows of one shape.  With stride = bnflac_out_stride(
 * out_format, sp), row s starts at d_rows + s * row_bytes: its first min(d_windows[s].nsamples,
 * row_samples) * stride bytes are the bytes of d_pcm from d_windows[s].pcm_first * stride, the rest
 * up to row_samples * stride is zero, and the bytes from there to row_bytes are not written.
 * d_pcm and d_rows are 16-byte aligned, d_pcm's allocation at least round_up(pcm_bytes, 16) bytes;
 * row_bytes is arbitrary but not below row_samples * stride (a negative return), and
 * BNFLAC_OUT_PLANAR32 (channel-major per frame) is refused (a negative return).  Any window table
 * will do, not only one bnflac_select_ranges wrote: a non-empty window that does not lie inside
 * pcm_bytes gives a zero row.  d_status (device, 4 words): [0] bit 0 some such window, [1] how
 * many, [2] rows cut at row_samples, [3] 0.  Nothing outside [0, round_up(pcm_bytes, 16)) is read.
 * Asynchronous on hip_stream, no host synchronisation, no allocation. */
BNFLAC_API int bnflac_gather_ranges(bnflac_ctx *ctx, const uint8_t *d_pcm, uint64_t pcm_bytes, int out_format,
                                    const bnflac_stream_params *sp, const bnflac_window *d_windows, uint32_t nstreams,
                                    uint32_t row_samples, uint64_t row_bytes, uint8_t *d_rows, uint32_t *d_status,
                                    void *hip_stream);

/* flags of bnflac_gather_ranges_f32 */
enum { BNFLAC_F32_MONO = 1 }; /* one plane per stream: the mean of the channels */

/* The windows of a decoded selection as normalised float32 channel planes: what bnflac_gather_ranges
 * does, with the layout conversion a device-side consumer needs in the same pass.
 * Layouts: exactly those for which bnflac_md5_layout(out_format, sp) is not 0, whose bytes are the
 * samples themselves: BNFLAC_OUT_INTERLEAVED32 (bps 4..32; an int32 per sample), BNFLAC_OUT_FLACDECODER
 * for 16-bit streams of 1-2 channels (an int16), BNFLAC_OUT_FILEREADER for 16- and 24-bit streams
 * (2 or 3 little-endian bytes, sign-extended).  With stride = bnflac_out_stride(out_format, sp) and
 * unit = stride / channels, sample (i, c) of window s is at byte (d_windows[s].pcm_first + i) *
 * stride + c * unit of d_pcm.  Every other layout, BNFLAC_OUT_PLANAR32 among them, is refused.
 * Values, bit for bit, with v the sample as int32 and k = 2^-(bps - 1):
 *   per channel:  f = (float)v * k.  The int -> float conversion rounds to nearest even (exact for
 *   |v| <= 2^24), the product with a power of two is exact, the smallest magnitude 2^-31 is normal.
 *   BNFLAC_F32_MONO:  f = (float)((double)S * k / channels), S the int64 sum of the sample frame's
 *   channels: an exact double product, one correctly rounded double division, one double -> float
 *   rounding.  For one channel this is the per-channel value.
 * Windows: the rule of bnflac_gather_ranges.  limit = pcm_bytes / stride; a window with nsamples != 0
 * and (pcm_first > limit or nsamples > limit - pcm_first) is bad: nothing of it is read, its planes
 * are zero, it is counted.  ncopy = min(nsamples, row_samples).  Any window table will do.
 * Output: planes = 1 with BNFLAC_F32_MONO, else channels.  Plane c of stream s starts at d_out +
 * (s * planes + c) * plane_pitch floats: its first ncopy floats are values, the rest up to
 * row_samples are +0.0f, and the floats from row_samples to plane_pitch are not written.
 * plane_pitch is any value not below row_samples (a contiguous [nstreams, planes, T] tensor with odd
 * T will do).  d_pcm and d_out are 16-byte aligned, d_windows 8-byte aligned, d_pcm's allocation at
 * least round_up(pcm_bytes, 16) bytes; nothing outside [0, round_up(pcm_bytes, 16)) is read.
 * d_status (device, 4 words): [0] bit 0 some bad window, [1] how many, [2] rows cut at row_samples,
 * [3] 0.  nstreams == 0 writes a zero status.
 * Refused (a negative return, the cause in bnflac_last_error(), nothing launched, nothing written):
 * a null argument as in bnflac_gather_ranges, a layout as above, channels outside 1..8, flag bits
 * other than BNFLAC_F32_MONO, plane_pitch < row_samples, a pointer less aligned than stated,
 * nstreams >= 2^30.
 * No trip count or address depends on a window's contents beyond the check above.  Asynchronous on
 * hip_stream, no host synchronisation, no allocation; the launch runs on ctx's device. */
BNFLAC_API int bnflac_gather_ranges_f32(bnflac_ctx *ctx, const uint8_t *d_pcm, uint64_t pcm_bytes, int out_format,
                                        const bnflac_stream_params *sp, const bnflac_window *d_windows, uint32_t nstreams,
                                        uint32_t row_samples, uint64_t plane_pitch, uint32_t flags, float *d_out,
                                        uint32_t *d_status, void *hip_stream);

/* The same planes and status from host memory, by the same code (csrc/bnf_pcm_f32.h); no GPU needed.
 * Refuses what the device call refuses apart from pointer alignment (out needs a float's).  0 or -1. */
BNFLAC_API int bnflac_gather_ranges_f32_host(const uint8_t *pcm, uint64_t pcm_bytes, int out_format,
                                             const bnflac_stream_params *sp, const bnflac_window *windows, uint32_t nstreams,
                                             uint32_t row_samples, uint64_t plane_pitch, uint32_t flags, float *out,
                                             uint32_t status[4]);

/* A rational rate change for bnflac_gather_ranges_f32_rs: rate_out / rate_in = up / down. */
typedef struct {
    uint32_t up, down;  /* L, M: rate_out / g, rate_in / g, g = gcd(rate_in, rate_out); coprime, 1..65535 */
    uint32_t taps;      /* K: taps per phase, a multiple of 4 in 4..512, up * taps <= 16384 */
    uint32_t out_first; /* output index of the window that lands in row position 0, below 2^31 */
} bnflac_resample_spec; /* 16 bytes */

/* bnflac_gather_ranges_f32 with the windows filtered to another sample rate in the same launch: a
 * polyphase FIR whose table the caller passes.  d_taps is a device table of spec->up * spec->taps
 * float32, phase-major: h[phase][k] at phase * taps + k.  The contract is in terms of the table's
 * float32 values, whoever made them (bnflac_resample_design makes a Kaiser-windowed sinc).
 * Layouts, the window check, the plane layout, MONO and the status words are those of
 * bnflac_gather_ranges_f32, with row_out in row_samples' place.  Per window s that passes the check,
 * with n its nsamples, L = up, M = down, K = taps: x[i] for 0 <= i < n is the float
 * bnflac_gather_ranges_f32 specifies for sample frame i of the plane ((float)v * 2^-(bps-1) for channel
 * c, or the mono rule with BNFLAC_F32_MONO), and x[i] = +0.0f for every other i.  A window is filtered
 * on its own: nothing outside it is read.
 *   n_out = max(0, ceil(n L / M) - out_first), ncopy = min(n_out, row_out).
 *   Row position r < ncopy is output j = r + out_first: q = floor(j M / L), phase = (j M) mod L,
 *   c0 = K / 2 - 1.  Four float32 accumulators start at +0.0f; for k = 0 .. K - 1 ascending
 *       a[k & 3] = fmaf(h[phase][k], x[q + k - c0], a[k & 3])        (one rounding per term)
 *   and the value is (a[0] + a[1]) + (a[2] + a[3]), each + one float32 addition.
 *   Row positions [ncopy, row_out) are +0.0f; floats from row_out to plane_pitch are not written.
 * Values are these bit for bit, on the device and in bnflac_gather_ranges_f32_rs_host.
 * d_status (device, 4 words): [0] bit 0 some bad window, [1] how many, [2] windows with n_out >
 * row_out, [3] 0.  nstreams == 0 writes a zero status.
 * Refused (a negative return, the cause in bnflac_last_error(), nothing launched, nothing written):
 * everything bnflac_gather_ranges_f32 refuses (layouts, channels outside 1..8, flag bits other than
 * BNFLAC_F32_MONO, plane_pitch < row_out, alignments, nstreams >= 2^30, null arguments); a null spec or
 * d_taps; up or down outside 1..65535 or not coprime; taps outside 4..512 or no multiple of 4;
 * up * taps > 16384; row_out or out_first not below 2^31; d_taps not 16-byte aligned.
 * spec is read on the host at call time.  No trip count or address depends on a window's contents
 * beyond the check.  Asynchronous on hip_stream, no host synchronisation, no allocation; the launch
 * runs on ctx's device.  The output tile is 1,024 row positions of one window. */
BNFLAC_API int bnflac_gather_ranges_f32_rs(bnflac_ctx *ctx, const uint8_t *d_pcm, uint64_t pcm_bytes, int out_format,
                                           const bnflac_stream_params *sp, const bnflac_window *d_windows, uint32_t nstreams,
                                           const bnflac_resample_spec *spec, const float *d_taps, uint32_t row_out,
                                           uint64_t plane_pitch, uint32_t flags, float *d_out, uint32_t *d_status,
                                           void *hip_stream);

/* The same planes and status from host memory, by the same code (csrc/bnf_resample.h); no GPU needed.
 * Refuses what the device call refuses apart from pointer alignment (out and taps need a float's).
 * 0 or -1. */
BNFLAC_API int bnflac_gather_ranges_f32_rs_host(const uint8_t *pcm, uint64_t pcm_bytes, int out_format,
                                                const bnflac_stream_params *sp, const bnflac_window *windows,
                                                uint32_t nstreams, const bnflac_resample_spec *spec, const float *taps,
                                                uint32_t row_out, uint64_t plane_pitch, uint32_t flags, float *out,
                                                uint32_t status[4]);

/* A table for bnflac_gather_ranges_f32_rs: a Kaiser-windowed sinc.  Host only, no GPU.  Fills spec
 * (out_first = 0), returns the floats the table needs, up * taps, and writes them to taps when
 * taps_cap is at least that (so a call with taps_cap = 0 sizes the table).  zeros: zero crossings of
 * the sinc on each side (default 16); rolloff: the cutoff as a fraction of the lower Nyquist
 * frequency (default 0.945); beta: the Kaiser window's (default 9.0); a value <= 0 means the default.
 * In double, with L = up, M = down:  s = min(1, L / M), fc = rolloff * s,
 * K = round_up(2 * ceil(zeros / s), 4), c0 = K / 2 - 1, tau = (k - c0) - phase / L,
 * w = I0(beta * sqrt(1 - (tau / (K/2))^2)) / I0(beta) for |tau| < K / 2, else 0,
 * g = fc * sinc(fc * tau) * w with sinc(x) = sin(pi x) / (pi x), h[phase][k] = (float)(g / sum_k g):
 * every phase has unit gain at DC.  Equal rates give {1, 1, 4} and the table {0, 1, 0, 0}, the identity.
 * A negative return for a zero rate, a null spec, or a table over the gather's limits; then
 * bnflac_last_error() states the up and taps the design needs, so a caller can lower zeros. */
BNFLAC_API int64_t bnflac_resample_design(uint32_t rate_in, uint32_t rate_out, double zeros, double rolloff, double beta,
                                          bnflac_resample_spec *spec, float *taps, uint64_t taps_cap);

/* The source window for outputs [j0, j0 + n_out) of a stream on the output-rate grid, with the
 * filter's whole support on both sides.  Host only.  With c0 = K / 2 - 1:
 *   b = max(0, floor(j0 M / L) - c0) / M (an integer division), first_sample = M b,
 *   out_first = j0 - L b, nsamples = floor((j0 + n_out - 1) M / L) + K / 2 + 1 - first_sample
 *   (0 for n_out = 0).
 * The window starts on a multiple of M, so its output grid is the stream's: a request of
 * (stream, first_sample, nsamples) and a spec with this out_first give the same values as the same
 * outputs of the whole stream, whose end the selection's clipping supplies.  spec's own out_first is
 * not read.  0, or -1 for a null argument, a spec the gather refuses or j0 + n_out >= 2^47. */
BNFLAC_API int bnflac_resample_request(const bnflac_resample_spec *spec, uint64_t j0, uint64_t n_out, uint64_t *first_sample,
                                       uint64_t *nsamples, uint32_t *out_first);

/* An STFT and band projection for bnflac_gather_ranges_mel. */
typedef struct {
    uint32_t n_fft;       /* N: a power of two, 64..2048 */
    uint32_t hop;         /* 1..65535 */
    uint32_t n_mels;      /* 0..256; 0: the rows are the n_fft/2 + 1 power-spectrum bins */
    int32_t origin;       /* sample index, relative to the window's sample 0, of tap 0 of frame 0;
                             -(n_fft/2) is torch.stft(center=True, pad_mode="constant") */
    uint32_t n_weights;   /* floats of the band weights, 0..8192; 0 when n_mels == 0 */
    uint32_t reserved[3]; /* 0 */
} bnflac_mel_spec;        /* 32 bytes */

/* flags of status word 0 of bnflac_gather_ranges_mel */
enum { BNFLAC_MEL_BAD_WINDOW = 1, BNFLAC_MEL_BAD_BAND = 2 };

/* The windows of a decoded selection as mel (or power) spectrogram planes [windows, planes, rows,
 * frames] in one launch: bnflac_gather_ranges_f32, a windowed STFT, the power and a band-sparse
 * projection, with the PCM read once and nothing but the feature tensor written.
 * Tables.  The contract is in terms of the tables' values, whoever made them (bnflac_mel_design makes
 * a Hann window, exact twiddles and HTK mel triangles).  With N = n_fft:
 *   d_tab   float32, 16-byte aligned: the analysis window w[0 .. N), then N/2 twiddle pairs
 *           C[k], S[k] at d_tab[N + 2k], d_tab[N + 2k + 1] for k = 0 .. N/2 - 1 (a design has
 *           C[k] = cos(2 pi k / N), S[k] = sin(2 pi k / N); the factor applied is C[k] - i S[k]),
 *           then the n_weights band weights: 2 N + n_weights floats.
 *   d_bands uint32, n_mels + 1 pairs {first_bin, woff}: band m covers bins first_bin[m] ..
 *           first_bin[m] + nb with nb = woff[m+1] - woff[m], its weights are weights[woff[m] ..].
 *           It may be NULL when n_mels == 0.  A band is bad if woff[m+1] < woff[m], if woff[m+1] >
 *           n_weights, or if first_bin[m] + nb > N/2 + 1.  A bad band is empty: its row is +0.0f,
 *           and it is counted once per launch.  Whatever the tables hold, the call returns some
 *           values and never faults: no trip count or address is a table value beyond that clamp.
 * Layouts, the window check, planes and BNFLAC_F32_MONO are those of bnflac_gather_ranges_f32.  Per
 * window s that passes the check, with n its nsamples: x[i] for 0 <= i < n is the float
 * bnflac_gather_ranges_f32 specifies for sample frame i of the plane, x[i] = +0.0f for every other
 * i.  Nothing outside the window is read.
 * Frames.  Frame t starts at a_t = origin + t * hop (signed 64-bit).  n_valid = 0 when n == 0 or
 * c = n - N/2 - origin < 0, else c / hop + 1: the frames whose centre lies at or before the window's
 * end (origin = -N/2 gives torch's 1 + n / hop).  ncopy = min(n_valid, row_frames).
 * Values of frame t < ncopy, every operation one float32 rounding, fmaf a fused multiply-add:
 *   1. u[i] = w[i] * x[a_t + i], i = 0 .. N - 1                       (one product)
 *   2. X = DFT_N(u) by the radix-2 decimation-in-time FFT on N complex points, no real-input
 *      packing: v[brev(i)] = (u[i], +0.0f), brev the reversal of log2 N bits; then the stages
 *      h = 1, 2, 4, .. N/2 in this order; in stage h, for every block base b (a multiple of 2h) and
 *      j = 0 .. h - 1, with k = j * (N / 2h), A = v[b + j], B = v[b + j + h]:
 *          pr = B.im * S[k];      tr = fmaf(B.re, C[k], pr)
 *          pi = B.re * S[k];      ti = fmaf(B.im, C[k], -pi)
 *          v[b + j]     = (A.re + tr, A.im + ti)
 *          v[b + j + h] = (A.re - tr, A.im - ti)
 *      The twiddles come from the table only, k = 0 included.  X[k] = v[k].
 *   3. P[k] = fmaf(re, re, im * im) with (re, im) = X[k], k = 0 .. N/2.
 *   4. n_mels == 0: row k is P[k].  Else row m: acc = +0.0f; for i = 0 .. nb - 1 ascending
 *      acc = fmaf(weights[woff[m] + i], P[first_bin[m] + i], acc); the row's value is acc.
 * No log: logf is not the same function on host and device, and the output is small enough for one
 * elementwise op downstream.  Values are these bit for bit, on the device and in
 * bnflac_gather_ranges_mel_host (tables without NaNs: a NaN's payload is not specified).
 * Output: rows = n_mels ? n_mels : N/2 + 1.  Row r of plane c of window s starts at d_out +
 * ((s * planes + c) * rows + r) * frame_pitch floats: its first ncopy floats are values, the rest up
 * to row_frames are +0.0f, floats from row_frames to frame_pitch are not written.  A bad window's
 * rows are all zero.
 * d_status (device, 4 words): [0] bit 0 some bad window, bit 1 some bad band, [1] bad windows,
 * [2] windows with n_valid > row_frames, [3] bad bands.  nstreams == 0 writes zeros.
 * Refused (a negative return, the cause in bnflac_last_error(), nothing launched, nothing written):
 * everything bnflac_gather_ranges_f32 refuses (layouts, channels outside 1..8, flag bits other than
 * BNFLAC_F32_MONO, alignments, nstreams >= 2^30, null arguments); a null spec or d_tab; d_bands null
 * with n_mels != 0; n_fft no power of two in 64..2048; hop outside 1..65535; n_mels above 256;
 * n_weights above 8192, or not 0 with n_mels == 0; a non-zero reserved word; row_frames not below
 * 2^31; frame_pitch < row_frames; d_tab not 16-byte aligned or d_bands not 4-byte aligned.
 * spec is read on the host at call time.  Trip counts: the tiles of a row by row_frames, the planes
 * and row passes by spec and the layout, the bins of a band by its clamped nb; a window enters through
 * the check and through ncopy alone: the frames computed in a tile are min(ncopy - tile start, 32),
 * a function of the window's nsamples bounded by row_frames and the same for every lane of a
 * workgroup, so a window without valid frames costs only its zero stores.  No address depends on a
 * window beyond the checked pcm_first.  Asynchronous on hip_stream, no host synchronisation, no
 * allocation; the launch runs on ctx's device.  The output tile is 32 frames of one window. */
BNFLAC_API int bnflac_gather_ranges_mel(bnflac_ctx *ctx, const uint8_t *d_pcm, uint64_t pcm_bytes, int out_format,
                                        const bnflac_stream_params *sp, const bnflac_window *d_windows, uint32_t nstreams,
                                        const bnflac_mel_spec *spec, const float *d_tab, const uint32_t *d_bands,
                                        uint32_t row_frames, uint64_t frame_pitch, uint32_t flags, float *d_out,
                                        uint32_t *d_status, void *hip_stream);

/* The same rows and status from host memory, by the same code (csrc/bnf_mel.h); no GPU needed.
 * Refuses what the device call refuses apart from pointer alignment (out, tab and bands need their
 * type's).  0 or -1. */
BNFLAC_API int bnflac_gather_ranges_mel_host(const uint8_t *pcm, uint64_t pcm_bytes, int out_format,
                                             const bnflac_stream_params *sp, const bnflac_window *windows, uint32_t nstreams,
                                             const bnflac_mel_spec *spec, const float *tab, const uint32_t *bands,
                                             uint32_t row_frames, uint64_t frame_pitch, uint32_t flags, float *out,
                                             uint32_t status[4]);

/* Tables for bnflac_gather_ranges_mel.  Host only, no GPU.  Fills spec (origin = -(n_fft/2), the
 * n_weights of the design), returns the floats tab needs, 2 n_fft + n_weights, and writes both tables
 * when tab_cap is at least that and bands_cap at least 2 (n_mels + 1) words (0 for n_mels == 0), so
 * a call with zero caps sizes them.  f_max <= 0 means sample_rate / 2.  In double, rounded to float:
 *   w[i] = 0.5 - 0.5 cos(2 pi i / N)                          (the periodic Hann window)
 *   C[k] = cos(2 pi k / N), S[k] = sin(2 pi k / N)
 *   mel(f) = 2595 log10(1 + f / 700), hz(m) = 700 (10^(m / 2595) - 1);
 *   f_j = hz(mel(f_min) + j (mel(f_max) - mel(f_min)) / (n_mels + 1)), j = 0 .. n_mels + 1;
 *   bin k has frequency g_k = k sample_rate / N; the weight of bin k in band m is
 *   max(0, min((g_k - f_m) / (f_m+1 - f_m), (f_m+2 - g_k) / (f_m+2 - f_m+1)))    (HTK, unnormalised):
 * torchaudio.functional.melscale_fbanks(norm=None, mel_scale="htk") with its zero weights dropped.
 * Band m holds the bins whose float32 weight is above 0, one run; a band without one has nb = 0 and
 * first_bin 0.  The last pair is {0, n_weights}.
 * A negative return for a zero rate, a null spec, sizes the gather refuses, f_min and f_max not
 * 0 <= f_min < f_max <= sample_rate / 2, or a design over the gather's limits; then
 * bnflac_last_error() states the n_mels and n_weights the design needs. */
BNFLAC_API int64_t bnflac_mel_design(uint32_t sample_rate, uint32_t n_fft, uint32_t hop, uint32_t n_mels, double f_min,
                                     double f_max, bnflac_mel_spec *spec, float *tab, uint64_t tab_cap, uint32_t *bands,
                                     uint64_t bands_cap);

/* The source window for frames [t0, t0 + n_frames) of a stream's own frame grid (frame t of the
 * stream starts at sample spec->origin + t * hop), with the whole support of every frame.  Host only.
 *   start = origin + t0 hop, first_sample = max(0, start), *origin = start - first_sample,
 *   nsamples = max(0, start + (n_frames - 1) hop + N - first_sample)  (0 for n_frames = 0).
 * A request of (stream, first_sample, nsamples) and a spec with this origin give the same values as
 * columns [t0, t0 + n_frames) of the whole stream's result, bit for bit: the stream's start is
 * supplied by the zero extension in front of the window, its end by the selection's clipping.
 * 0, or -1 for a null argument, a spec the gather refuses or t0 + n_frames >= 2^31. */
BNFLAC_API int bnflac_mel_request(const bnflac_mel_spec *spec, uint64_t t0, uint64_t n_frames, uint64_t *first_sample,
                                  uint64_t *nsamples, int32_t *origin);

/* ======================== Part 3: streaming reader ======================= */

/* The fast path under FLACDecoder.Read (FLACDecoder.cs:124-205) and OpenAL's buffer fill
 * (OpenALDemo/Program.cs:33-38): a whole FLAC stream in host memory in, packed PCM out in
 * caller-sized pieces.  open() copies the stream to HBM once, indexes its frames on the GPU
 * (bnflac_index_stream) and starts decoding ahead in windows of `window_frames` frames
 * (0: 256) into a two-slot pinned host ring; read() copies from the ring while the next
 * window decodes.  The bytes are those of out_format (BNFLAC_OUT_FLACDECODER: what
 * FLACDecoder.CopyTo yields).  Intact streams only: open() or read() returns -1 at the
 * first sign of damage (frame chain short of STREAMINFO's total, CRC failure), with the
 * reason in bnflac_reader_last_error(); the libFLAC stream API (part 1) handles those. */
typedef struct bnflac_reader bnflac_reader;
BNFLAC_API int bnflac_reader_open(int device, const uint8_t *bytes, uint64_t nbytes, int out_format,
                                  uint32_t window_frames, bnflac_reader **out);
/* STREAMINFO, total PCM bytes the reader will return, frames found.  Any pointer may be NULL. */
BNFLAC_API int bnflac_reader_params(const bnflac_reader *reader, bnflac_stream_params *sp, uint64_t *total_bytes,
                                    uint32_t *nframes);
/* Up to count bytes into buf; returns the number copied (0: end of stream) or -1. */
BNFLAC_API int64_t bnflac_reader_read(bnflac_reader *reader, uint8_t *buf, uint64_t count);
/* Position the reader so the next read starts at `sample` (per channel), like
 * FLACFileReader.Position / seek_absolute (FLACFileReader.cs:109-137,295-299).  0 or -1
 * (sample past the end, or damage in the target window). */
BNFLAC_API int bnflac_reader_seek(bnflac_reader *reader, uint64_t sample);
/* FLACFileReader.Read(buffer, offset, numBytes) (FLACFileReader.cs:145-254) replayed with
 * buffer.Length = buffer_length, on a reader opened with BNFLAC_OUT_FILEREADER: samples left
 * over from the previous call first, then whole frames until numBytes are reached; every copy
 * runs to the buffer's end (the return may exceed num_bytes), m_samplesPerChannel is the first
 * frame's blocksize (shorter frames leave earlier samples behind, longer ones are cut).
 * Returns the bytes copied, 0 at the end, -1 with the C# exception's message in
 * bnflac_reader_last_error() ("Index was outside the bounds of the array." / "Input FLAC bit
 * depth is not supported!").  Not mixed with bnflac_reader_read / bnflac_reader_seek. */
BNFLAC_API int64_t bnflac_reader_read_filereader(bnflac_reader *reader, uint8_t *buffer, uint64_t offset,
                                                 uint64_t num_bytes, uint64_t buffer_length);
BNFLAC_API void bnflac_reader_close(bnflac_reader *reader);
/* A closed reader's stream, events and small buffers stay pooled per device for the next
 * open (buffers above BNFLAC_READER_POOL_CAP bytes, default 64 MiB, are freed on close;
 * BNFLAC_READER_POOL=0 turns pooling off).  This frees every pooled resource of `device`
 * (-1: of every device), e.g. before handing the GPU's memory to another user.  Returns the
 * number of pooled reader sets freed. */
BNFLAC_API int bnflac_reader_pool_release(int device);
BNFLAC_API const char *bnflac_reader_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* BNFLAC_H */
