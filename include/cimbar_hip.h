/* cimbar_hip.h -- C ABI of the MI355X (gfx950) cimbar mode-B frame-decode path.
 *
 * Drop-in boundary: everything between "a deskewed 1024x1024 RGB8 frame" and "the <=12 fountain chunks of 625 bytes
 * that libcimbar hands to fountain_decoder_sink::write". It replaces, for that path only, what the reference does in
 *     Decoder::decode_fountain            /root/reference/src/lib/encoder/Decoder.h:171-189 (-> do_decode :60-118)
 *     CimbReader / CimbDecoder            src/lib/cimb_translator/CimbReader.cpp:107-280, CimbDecoder.cpp:101-217
 *     reed_solomon_stream / aligned_stream src/lib/encoder/reed_solomon_stream.h:54-77, aligned_stream.h:39-119
 * and mirrors the shape of the reference's own C ABI for the same step,
 *     cimbard_get_bufsize / cimbard_scan_extract_decode / cimbard_configure_decode
 *                                          src/lib/cimbar_js/cimbar_recv_js.h:16-17,36; cimbar_recv_js.cpp:143-189
 * (minus the Scanner/Extractor call, which is upstream of this path).
 *
 * Conventions: plain C types, caller-allocated buffers, no exceptions across the boundary. Functions returning int
 * return >= 0 on success and a negative CIMBAR_HIP_E* code on failure. One context serves one host thread at a time
 * and carries the colour-correction matrix from frame to frame exactly like the reference's `static thread_local`
 * CCM (CimbDecoder.cpp:69-73). There is NO CPU fallback: if no gfx950 device/kernel image is usable, create() fails.
 */
#ifndef CIMBAR_HIP_H
#define CIMBAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CIMBAR_HIP_FRAME_DIM 1024          /* Conf8x8 image_size_x/y, GridConf.h:130-131 */
#define CIMBAR_HIP_CELLS 12400             /* GridConf.h:42-45 */
#define CIMBAR_HIP_CHUNK_SIZE 625          /* Config::fountain_chunk_size(), GridConf.h:63-71 */
#define CIMBAR_HIP_CHUNKS_PER_FRAME 12     /* Config::fountain_chunks_per_frame(6), GridConf.h:54-61 */
#define CIMBAR_HIP_FRAME_BYTES (CIMBAR_HIP_CHUNK_SIZE * CIMBAR_HIP_CHUNKS_PER_FRAME) /* 7500 = cimbard_get_bufsize() in mode B -- MODE B ONLY */
/* The largest chunk space any mode's frame needs: mode 8 (the legacy 8-colour mode) delivers 10 chunks of 875 bytes = 8750 (modes 68 / 4:
 * 7500, 67: 5148, 66: 3240). Size fixed buffers with THIS, or ask cimbar_hip_ctx_bufsize(ctx) -- never with CIMBAR_HIP_FRAME_BYTES unless the
 * context is known to be mode B's. */
#define CIMBAR_HIP_MAX_FRAME_BYTES 8750

enum {
	CIMBAR_HIP_OK = 0,
	CIMBAR_HIP_EINVAL = -1,       /* bad argument (null pointer, n <= 0, unsupported mode) */
	CIMBAR_HIP_EDIM = -2,         /* frame is not 1024x1024 RGB8 (cf. CimbReader::_good, CimbReader.cpp:119) */
	CIMBAR_HIP_ENODEVICE = -3,    /* no usable gfx950 device / kernel image */
	CIMBAR_HIP_EHIP = -4,         /* a HIP runtime call failed; see cimbar_hip_last_error() */
	CIMBAR_HIP_ENOMEM = -5
};

/* where a buffer argument lives */
enum { CIMBAR_HIP_MEM_HOST = 0, CIMBAR_HIP_MEM_DEVICE = 1 };

typedef struct cimbar_hip_ctx cimbar_hip_ctx;

/* cimbard_configure_decode(mode) + `Decoder dec;` (cimbar_recv_js.cpp, Config::update, Config.h:19-50). Modes built: 68 ("B", Conf8x8,
 * 1024x1024, GridConf.h:121-142; 0 selects it too, Config::temp_conf's default), 67 ("Bm", Conf8x8_mini, 1024x720, GridConf.h:168-189) and
 * 66 ("Bu", Conf8x8_micro, 736x637, GridConf.h:144-166), and 4 (the legacy 4-colour mode, Config.h:24-29: mode B's grid with the coupled decode
 * of Decoder.h:121-161 -- one Reed-Solomon stream of 6-bit cells, the old palette, no header-derived colour correction) and 8 (the legacy
 * 8-colour mode, Config.h:30-35: 7-bit cells, 70 blocks, 10 * 875 bytes) -- every mode Config::temp_conf knows. Any other value selects mode
 * 68, exactly like Config::temp_conf's `default:` branch (Config.h:41-43): cimbard_configure_decode(5) upstream gives a working mode-B
 * decoder, and so does cimbar_hip_create(dev, 5) (cimbar_hip_geometry then reports mode 68). `device` is a HIP device ordinal. Everywhere below "frame" means an
 * image_size_x x image_size_y RGB8 image of the context's mode, "12 * 625" the mode's chunks-per-frame * chunk size (12 * 429 in mode 67,
 * 6 * 540 in mode 66, 10 * 750 in mode 4; the mask has as many bits) and "60 blocks of 125" its RS layout (36 of 143; 24 of 135):
 * cimbar_hip_geometry reports the numbers. */
int cimbar_hip_create(int device, int mode_val, cimbar_hip_ctx** out);
void cimbar_hip_destroy(cimbar_hip_ctx* ctx);

/* cimbard_get_bufsize() (cimbar_recv_js.cpp:143-146) = fountain_chunks_per_frame() * fountain_chunk_size() of the ACTIVE configuration. The
 * reference's configuration is a thread_local; here it lives in the context, so the faithful counterpart takes one:
 *   cimbar_hip_ctx_bufsize(ctx) : the chunk space one frame of THIS context needs (7500 / 5148 / 3240 / 7500 / 8750 for modes 68 / 67 / 66 / 4 / 8)
 *   cimbar_hip_bufsize()        : the same for the default configuration (mode B, what a thread that never called Config::update has): 7500
 *   cimbar_hip_mode_bufsize(m)  : the same for the configuration cimbard_configure_decode(m) selects, without a context or a device (what a
 *                                 cimbard_get_bufsize() replacement answers before the first frame arrives: libcimbar_recv_hip.so) */
int cimbar_hip_ctx_bufsize(const cimbar_hip_ctx* ctx);
int cimbar_hip_bufsize(void);
int cimbar_hip_mode_bufsize(int mode_val);

/* The grid a context was created for -- the Config:: getters the reference's callers size their buffers with (Config.h:52-165):
 * out = {mode, image_size_x, image_size_y, total_cells, fountain_chunks_per_frame, fountain_chunk_size, RS blocks per frame (symbol + colour),
 *        ecc_block_size, ecc_bytes, cells_per_col_x, cells_per_col_y, cell_offset}. Returns CIMBAR_HIP_GEOMETRY_WORDS. */
enum { CIMBAR_HIP_GEOMETRY_WORDS = 12 };
int cimbar_hip_geometry(const cimbar_hip_ctx* ctx, int32_t out[CIMBAR_HIP_GEOMETRY_WORDS]);

/* The 16 symbol-tile hashes as cimbar_hip_create computes them from the embedded tile bitmaps -- what CimbDecoder's constructor does
 * (CimbDecoder.cpp:58-66,87-99: getTile -> average_hash). Host-only arithmetic (works without a device); returns 16. */
int cimbar_hip_tile_hashes(uint64_t out16[16]);

/* the HIP device ordinal the context lives on */
int cimbar_hip_device(const cimbar_hip_ctx* ctx);

/* human-readable text of the last failure on this context (never NULL) */
const char* cimbar_hip_last_error(const cimbar_hip_ctx* ctx);

/* Decoder::decode_fountain(img, sink, should_preprocess, color_correction) for ONE host-resident frame.
 *   rgb        : height rows of `stride` bytes, width*3 used (RGB8, as cv::Mat CV_8UC3 after BGR2RGB, cimbar.cpp:132-133)
 *   chunks     : cimbar_hip_ctx_bufsize(ctx) bytes (12*625 in mode B; at most CIMBAR_HIP_MAX_FRAME_BYTES); slot j holds fountain chunk j of the
 *                frame, zero-filled if the chunk was dropped
 *   good_mask  : bit j set <=> aligned_stream delivered chunk j to the sink (aligned_stream.h:62-85)
 * Returns the reference's return value: cumulative good bytes = 625 * popcount(mask) (Decoder.h:116-117).
 * Image size, as CimbReader's constructor treats it (CimbReader.cpp:107-126):
 *   width x height == image_size_x x image_size_y : the ordinary case (and the only one the batch entry points take);
 *   larger in either direction : the grid sits _gridPadding = min(width - image_size_x, height - image_size_y) / 2 pixels in, in x and in y, and
 *                                the threshold pass sees the real pixels around it (a single-image path, not tuned for throughput);
 *   smaller : the reference reads no cell at all, Reed-Solomon then "decodes" its all-zero buffers and every chunk is delivered as zeros --
 *             the call returns the full byte count, mask 0xFFF and zero-filled chunks, exactly like the reference (a fountain sink drops them). */
int cimbar_hip_decode_frame(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, size_t stride,
                            int should_preprocess, int color_correction, uint8_t* chunks, uint32_t* good_mask);

/* The same call with frames in flight -- the shape of the reference's decode loop (cimbar.cpp:124-171: one Decoder::decode_fountain per image,
 * the next image being read while this one decodes) and of web/recv-worker.js's frames-keep-arriving loop: frame k+1's host-to-device copy
 * runs beside frame k's kernels, so one context sustains the PCIe copy rate instead of copy + kernels + copy-back per frame.
 *   cimbar_hip_decode_frame_async : starts the frame and returns a ticket >= 0 (negative: an error code, nothing started). At most
 *                     cimbar_hip_pipeline_depth(ctx) frames are in flight; starting one more first completes the oldest (its chunks and mask land
 *                     in the buffers it was started with; its return value stays available to _wait for the next 16 tickets).
 *                     `rgb` in page-locked memory (hipHostMalloc / hipHostRegister) is copied from where it lies and must stay untouched until the
 *                     frame's _wait; pageable memory has been consumed when the call returns (a dense image through the runtime's own pageable copy, a
 *                     strided one -- a cv::Mat ROI -- through the context's page-locked staging) and may be reused or freed at once. `chunks` / `good_mask` are written by _wait (or by the completion described above), never before.
 *                     Images of another size than the frame (CimbReader.cpp:107-126's padded / too-small cases) are decoded synchronously behind
 *                     everything in flight and still get a ticket.
 *   cimbar_hip_decode_frame_wait  : blocks until that frame is complete and returns what cimbar_hip_decode_frame would have returned.
 * Frames are decoded in ticket order (the colour-correction matrix carries over from frame to frame exactly as in the synchronous call), so
 * waiting in ticket order hands the chunks to a sink in the order the reference's loop would. cimbar_hip_decode_frame IS _async + _wait.
 * Mixing with the batch entry points on one context: the frame slots ride on the pipeline's streams and scratch sets and are ordered among
 * themselves and behind cimbar_hip_decode_batch_pipelined; a batch call with DEVICE outputs on a stream of the caller's only enqueues, shares the
 * carried matrix and the flood scratch with the frame slots and is NOT ordered against them -- synchronise that stream before the next
 * cimbar_hip_decode_frame_async (a batch call with host outputs has synchronised when it returns). */
long long cimbar_hip_decode_frame_async(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, size_t stride,
                                        int should_preprocess, int color_correction, uint8_t* chunks, uint32_t* good_mask);
int cimbar_hip_decode_frame_wait(cimbar_hip_ctx* ctx, long long ticket);

/* The same for `n` independent frames, decoded in frame order (frame f's CCM carry-over sees frames < f).
 *   rgb        : n densely packed 1024*1024*3 frames, in host or device memory (rgb_mem)
 *   chunks     : n*7500 bytes, masks: n words, in host or device memory (out_mem)
 *   hip_stream : a hipStream_t to enqueue on. NULL = the null stream when a device buffer is involved (ordinary HIP
 *                semantics: ordered after the work that produced the frames there), the context's own stream when
 *                everything is host memory. With device outputs the call only enqueues work and returns 0; the caller
 *                synchronises the stream. With host outputs it synchronises and returns the total good bytes over the batch.
 */
int64_t cimbar_hip_decode_batch(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess,
                                int color_correction, uint8_t* chunks, uint32_t* masks, int out_mem, void* hip_stream);

/* A continuous stream of batches (device buffers only): the same work and the same results as cimbar_hip_decode_batch, but the call only
 * records "the frames are ready" on `hip_stream` and runs the batch on one of D = cimbar_hip_pipeline_depth() streams the context owns,
 * consecutive batches on consecutive streams. Up to D batches are then in flight at once and the threshold pass of one batch -- the
 * HBM-bound 70 % of the work -- overlaps the short, latency-bound kernels of the others; the colour-correction matrix still carries
 * over from batch to batch in order (a batch's colour pass waits for the end of the batch before it). The reference's receive loop has
 * the same shape: frames keep arriving while earlier ones are decoded (cimbar_recv_js.cpp:143-189 under web/recv.js's worker pool).
 * Contract: at most D batches in flight; the rgb / chunks / masks buffers of a batch must stay untouched until a
 * cimbar_hip_pipeline_wait that covers it has been enqueued and reached. Any other entry point of the context waits for the pipeline.
 *   cimbar_hip_pipeline_wait(ctx, stream, keep_newest): `stream` waits for every pipelined batch issued so far except the `keep_newest`
 *   most recent ones (0 = all of them; D-1 = only the oldest that can still be in flight: consume batch k-D+1 right after issuing
 *   batch k and the pipeline stays full). Enqueue-only, returns 0. */
int cimbar_hip_decode_batch_pipelined(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int should_preprocess, int color_correction,
                                      uint8_t* chunks, uint32_t* masks, void* hip_stream);
int cimbar_hip_pipeline_wait(cimbar_hip_ctx* ctx, void* hip_stream, int keep_newest);
int cimbar_hip_pipeline_depth(const cimbar_hip_ctx* ctx);

/* Decoder::decode(img, ostream, should_preprocess, color_correction) (src/lib/encoder/Decoder.h:163-169) -- the `./cimbar --no-fountain`
 * path (cimbar.cpp:270-272) -- for n frames: no aligned_stream, every 125-byte Reed-Solomon output is written where it falls and a
 * block libcorrect could not decode is written as 125 zero bytes (reed_solomon_stream.h:62-74,96-107).
 *   bytes    : n * 7500 bytes (60 blocks of 125 per frame: 40 from the symbol bits, then 20 from the colour bits)
 *   block_ok : n * 60 bytes, 1 = the block decoded; may be NULL. Same memory kind as `bytes`.
 * No fountain header reaches the reader on this path, so color_correction == 2 keeps whatever matrix the context carries
 * (CimbReader.cpp:169-180). Host outputs: synchronises and returns n * 7500 (what the stream's tellp() advanced by, Decoder.h:116-117);
 * device outputs: enqueues and returns 0. Buffers, stream and errors as for cimbar_hip_decode_batch. */
int64_t cimbar_hip_decode_plain_batch(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess,
                                      int color_correction, uint8_t* bytes, uint8_t* block_ok, int out_mem, void* hip_stream);

/* Clears the carried colour-correction state (what a fresh thread starts with in the reference). */
int cimbar_hip_reset_ccm(cimbar_hip_ctx* ctx);
/* Current carried CCM, row-major 3x3; returns 1 if active, 0 if not (CimbDecoder::get_ccm, CimbDecoder.cpp:76-80). */
int cimbar_hip_get_ccm(cimbar_hip_ctx* ctx, float out9[9]);
/* CimbDecoder::update_color_correction (CimbDecoder.cpp:82-85; what DecoderPlus::load_ccm feeds from `--color-correction-file`,
 * DecoderPlus.h:32-45, cimbar.cpp:265-266): the carried matrix becomes m9 (row-major 3x3) and is active from the next frame on, until a frame
 * derives its own (color_correction 2 with a decoded header) or cimbar_hip_reset_ccm. Waits for batches in flight. */
int cimbar_hip_set_ccm(cimbar_hip_ctx* ctx, const float m9[9]);

/* Erasure decoding (off after cimbar_hip_create). With sym_distance > 0, every decode entry point that reports chunks (decode_frame, _async,
 * decode_batch, _pipelined, scan_extract_decode_batch(_fmt), scan_undistort_extract_decode_batch_fmt) retries the symbol chunks its mask
 * lacks: a cell whose 8x8 hash at its final position is sym_distance or more bits from its decoded symbol's tile makes the stream bytes it
 * supplies erasures (at most max_erasures per block, the most distant first), the blocks errors-only decoding failed are decoded again with
 * them (cimbar_hip_rs_decode_erasures below), and a chunk whose blocks are then all accepted joins the mask with its bytes. Chunks already in
 * the mask, colour chunks, the per-block flags and the colour-correction state are never changed; the mask only gains bits.
 *   sym_distance  : <= 0 turns it off (nothing extra is launched); 1 .. 64 the threshold
 *   colour_margin : kept and reported, not used: the colour blocks have a retry and a setting of their own,
 *                   cimbar_hip_set_colour_erasure_decode below
 *   max_erasures  : < 0 = the default, parity - 8 (22 / 28 / 25 in modes 68 / 67 / 66); at most the parity bytes
 * Modes 4 and 8 (one coupled stream) refuse it (EINVAL); cimbar_hip_decode_plain_batch returns EINVAL while it is on. Takes effect for
 * batches issued after the call. get: writes the three values in force (max_erasures resolved), returns 1 if on, 0 if off. */
int cimbar_hip_set_erasure_decode(cimbar_hip_ctx* ctx, int sym_distance, int colour_margin, int max_erasures);
int cimbar_hip_get_erasure_decode(cimbar_hip_ctx* ctx, int* sym_distance, int* colour_margin, int* max_erasures);

/* The relaxed flood (off after cimbar_hip_create; modes 68 / 67 / 66). A frame that leaves the parallel symbol pass and that the certifying pass
 * does not settle is normally replayed in the reference's exact flood order, 12 400 dependent steps. With threshold >= 0 such a frame is flooded
 * in parallel rounds instead: a round decodes every offered cell whose best offer has a priority (its neighbour's match distance) of at most
 * max(threshold, the smallest priority on offer), each at the drift of the best offer it holds, smallest (priority, offering cell) first. That is
 * the reference's rule without its tie order, so symbols and drift may differ from the reference's in single cells. The result of a frame is
 * accepted when every one of its symbol RS blocks decodes; with fallback != 0 every other frame is replayed exactly inside the same call, and
 * its outputs are then the default policy's byte for byte. An accepted frame's colour pass reads at the relaxed drift, so its colour chunks may
 * differ from the default policy's in either direction. Whether the certifying pass settles a frame is not a function of the frame alone: it
 * declines on the first rule that fires, and on frames with large flat areas (a saturated disc of glare) that can depend on the order in which
 * its lanes queued tied cells. The default policy's outputs are the same either way; with the relaxed flood on, such a frame is flooded exactly
 * in one run and in rounds in another, so its CIMBAR_HIP_TAP_FLOOD_PATH, the stats below and an accepted frame's colour chunks may vary.
 *   threshold : -1 turns it off (nothing extra is launched); 0 .. 32 turns it on. CIMBAR_HIP_RELAXED_FLOOD_SUGGESTED (12) is the value of the
 *               table in DESIGN_WIDENING.md "Relaxed flood": the exact flood's quality in 40 .. 1 000 rounds; 24 and more degrade on shifted and
 *               rescaled frames, 0 .. 8 need thousands of rounds on noisy ones. Anything else is CIMBAR_HIP_EINVAL
 *   fallback  : != 0: frames with a failing symbol block take the exact replay (and the symbol RS pass runs a second time over the batch)
 * Modes 4 and 8 refuse threshold >= 0 (EINVAL): their one RS stream is decoded after the colour pass, so there is nothing to check the flood
 * against. Takes effect for batches issued after the call. get: writes the two values, returns 1 if on, 0 if off.
 * stats: out[0] frames flooded in rounds, [1] of those, frames whose symbol blocks all decoded, [2] frames handed to the exact replay (0 without
 * fallback), [3] rounds in total; cumulative over the batches issued since the last cimbar_hip_set_relaxed_flood, which clears them. */
#define CIMBAR_HIP_RELAXED_FLOOD_SUGGESTED 12
int cimbar_hip_set_relaxed_flood(cimbar_hip_ctx* ctx, int threshold, int fallback);
int cimbar_hip_get_relaxed_flood(cimbar_hip_ctx* ctx, int* threshold, int* fallback);
int cimbar_hip_relaxed_flood_stats(cimbar_hip_ctx* ctx, int64_t out[4]);

/* Colour erasure decoding (off after cimbar_hip_create; independent of cimbar_hip_set_erasure_decode: either, both or neither may be on). With
 * colour_margin > 0 the same entry points retry the COLOUR chunks a frame's mask lacks, after the symbol retry where that runs. A cell's
 * confidence is the classifier's margin: (second-smallest) - (smallest) squared distance of CimbDecoder::get_best_color, computed from the
 * mean and the matrix the colour pass classified the cell from (130 050 for pure green, cyan and yellow, 390 150 for pure magenta, 0 for
 * white, black, grey and every tie).
 * A colour-stream byte comes from four cells; it is flagged when one of them has a margin below colour_margin, the flagged bytes with the
 * smallest margins become erasures (at most max_erasures per block, ties to the lower byte position), and retry and acceptance are those of
 * the symbol retry. Chunks already in the mask, symbol chunks, the per-block flags, the colours and the colour-correction state are never
 * changed; the mask only gains bits. In the combined calls the group outputs pick up what the members' retry delivered.
 *   colour_margin : <= 0 turns it off (nothing extra is launched); CIMBAR_HIP_COLOUR_MARGIN_SUGGESTED is the value the tests use, chosen on
 *                   rendered frames (DESIGN_WIDENING.md "Colour erasure decoding"); camera captures are unmeasured
 *   max_erasures  : < 0 = the default, parity - 8; at most the parity bytes (else EINVAL)
 * Modes 4 and 8 refuse a positive margin (EINVAL); cimbar_hip_decode_plain_batch returns EINVAL while it is on. Takes effect for batches
 * issued after the call. get: writes the values in force (max_erasures resolved), returns 1 if on, 0 if off. */
#define CIMBAR_HIP_COLOUR_MARGIN_SUGGESTED 32512
int cimbar_hip_set_colour_erasure_decode(cimbar_hip_ctx* ctx, int colour_margin, int max_erasures);
int cimbar_hip_get_colour_erasure_decode(cimbar_hip_ctx* ctx, int* colour_margin, int* max_erasures);

/* Errors-and-erasures Reed-Solomon decode of n caller-given blocks of the context's code (RS(155,125) in modes 68 / 4 / 8, RS(179,143) in
 * 67, RS(168,135) in 66): libcorrect's correct_reed_solomon_decode_with_erasures, bit-exact, plus an acceptance check libcorrect does not
 * make. With e erasures a block decodes whenever 2 * (errors outside them) + e <= parity.
 *   blocks    : n * block_length bytes, transmit order
 *   erasures  : n * block_length bytes; the first counts[b] bytes of row b are byte positions (< block_length) in block b
 *   counts    : n bytes, the erasure count per block; a count above the parity bytes fails the block (libcorrect returns -1)
 *   msgs      : n * message_length bytes: libcorrect's output where status >= 0, the received message bytes where status is -1
 *   status    : n bytes, -1 = libcorrect returns -1; 0 = libcorrect returns the message but the corrected block is not a codeword, or a root
 *               of the locator lies in the shortened code's zero padding (a miscorrection); 1 = decoded and accepted
 *   mem       : CIMBAR_HIP_MEM_HOST (every buffer in host memory: staged through a buffer the context keeps, on hip_stream or the
 *               context's stream if NULL; synchronises) or CIMBAR_HIP_MEM_DEVICE (all on the device: enqueues on hip_stream, the null stream if
 *               NULL, and returns 0) -- the stream convention of cimbar_hip_encode_batch
 * Touches no decode state of the context. */
int cimbar_hip_rs_decode_erasures(cimbar_hip_ctx* ctx, const uint8_t* blocks, int n, const uint8_t* erasures, const uint8_t* counts, int mem,
                                  uint8_t* msgs, int8_t* status, void* hip_stream);

/* Multi-capture decoding. A camera captures each displayed frame several times; glare, blur and focus hit different cells in each capture.
 * These calls decode a batch capture by capture exactly as cimbar_hip_decode_batch / cimbar_hip_scan_extract_decode_batch_fmt do (chunks,
 * masks and status equal theirs for the same input and context settings, the colour-correction carry included), then decode every run of
 * captures of one frame (a "group") once more from the cells of all its members together.
 *   grouping     groups_in == NULL: agree(k, k+1) = the cells whose symbol and colour are both equal in captures k and k+1. Walking left to
 *                right, capture k starts a new group when it is the first, when agree(k-1, k) * 1000 < min_agree_permille * cells, when the
 *                previous group already has max_group members, or when capture k-1 or k is unusable (capture path: its extraction failed).
 *                Unusable captures are in no group (-1); groups are numbered 0, 1, ... in capture order. These calls' groups do not span two calls;
 *                the stream calls below carry the open group from call to call.
 *                groups_in != NULL (host memory, n ints): the caller's groups -- each -1 or an id, ids starting at 0 and rising by one, each
 *                id's captures contiguous and at most max_group; anything else is CIMBAR_HIP_EINVAL. On the capture path a capture whose
 *                extraction failed is left out of its group (and reported -1); a group left without members delivers nothing.
 *   min_agree_permille <= 0: 750 (a torn capture, half one frame and half the next, joins neither neighbour; two different frames agree on
 *                about 1/64 of the cells in mode 68). max_group <= 0: 4; above 8: CIMBAR_HIP_EINVAL.
 *   combined cells  per cell, over the members c with decisions s_c / col_c and d_c(t) = popcount(H_c ^ tile t), H_c the cell's 8x8 hash in
 *                member c's bit plane at its final position: the symbol is kept where all s_c agree, else argmin_t sum_c (2 d_c(t) - [t == s_c])
 *                (ties: lowest t; margin = second-lowest score - lowest); the colour is the plurality of col_c, a tie going to the colour of the
 *                tied member with the smallest d_c(symbol), then the lowest member index. A group of one capture, or of identical ones,
 *                reproduces that capture's cells.
 *   group decode the combined cells go through the same Reed-Solomon decode and chunk delivery as one frame (modes 4 / 8: the coupled
 *                stream); no colour-correction matrix is derived, read or carried. Group chunk j = the combined decode's chunk j where it
 *                delivered it, else chunk j of the lowest-index member that delivered it; gmask = the combined mask | the members' masks.
 *                With erasure decoding on (cimbar_hip_set_erasure_decode, modes 68 / 67 / 66) the symbol chunks still missing are retried
 *                with the stream bytes of symbol-disputed cells as erasures (smallest margin first, then stream position, at most
 *                max_erasures per block), accepted as in the per-capture retry; colour chunks are not retried in the group decode (with
 *                cimbar_hip_set_colour_erasure_decode on, the members' own colour retry runs before the group fill, which takes its chunks).
 *   chunks / masks / status  per capture, as for the plain call; groups_out: n ints (may be NULL)
 *   gchunks / gmasks         n slots of 12 * 625 bytes / one mask; slots at or above the group count are zero
 *   n_groups                 the group count (may be NULL)
 * Every output follows out_mem. Host outputs: synchronises and returns the group count. Device outputs: enqueues only (the grouping runs on
 * the device; nothing waits), writes the count to device memory and returns 0. Buffers, stream and errors as for cimbar_hip_decode_batch. */
int64_t cimbar_hip_decode_batch_combined(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                         const int* groups_in, int min_agree_permille, int max_group, uint8_t* chunks, uint32_t* masks,
                                         int* groups_out, uint8_t* gchunks, uint32_t* gmasks, int* n_groups, int out_mem, void* hip_stream);
int64_t cimbar_hip_scan_extract_decode_batch_combined_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n,
                                                          int img_mem, int preprocess, int color_correction, const int* groups_in,
                                                          int min_agree_permille, int max_group, uint8_t* chunks, uint32_t* masks, int* status,
                                                          int* groups_out, uint8_t* gchunks, uint32_t* gmasks, int* n_groups, int out_mem,
                                                          void* hip_stream);

/* Colour vote in the group decode (off after cimbar_hip_create). The group decode above settles a disputed colour by counting heads, and in a
 * group of two every colour disagreement is a tie. With the vote on, cimbar_hip_decode_batch_combined and
 * cimbar_hip_scan_extract_decode_batch_combined_fmt weigh each member's colour by the classifier's confidence in it instead. For one cell whose
 * members' colours differ (a "colour dispute"):
 *   marg_c   = member c's classifier margin, exactly what CIMBAR_HIP_TAP_COLOUR_MARGIN defines (the mean and the matrix its colour pass
 *              classified the cell from); w_c = marg_c + 1, so that a zero-margin member still decides between colours nobody else voted for
 *   score(k) = the sum of w_c over the members whose colour is k; the group colour is the k with the largest score, ties to the lowest k
 *   gm       = the largest score minus the second-largest (a colour nobody voted for scores 0): the group colour margin
 * A cell whose members agree on the colour is settled as before and has no margin. The group's symbols, the symbol margin, the per-capture
 * outputs and the colour-correction state do not depend on the setting; only the colour of colour-disputed cells can change, and with it the
 * group's colour chunks.
 * Group colour retry: with cimbar_hip_set_colour_erasure_decode(colour_margin, max_erasures) on as well, the colour chunks gmask still lacks
 * after the group fill are retried on the voted cells: a colour-stream byte's score is max over its four cells of colour_margin - gm (a cell
 * without a colour dispute contributes nothing), flagged when > 0, the max_erasures highest scores become erasures (ties to the lower byte),
 * and retry, acceptance and the mask update are the per-capture colour retry's. Chunks already in gmask are never rewritten. There is no
 * second threshold; with the vote on and the colour erasure setting off only the vote changes.
 * Modes 4 and 8 refuse on != 0 (EINVAL): the coupled stream has no colour chunks of its own. This setting governs the plain combined calls
 * only: the stream calls below (..._combined_stream) behave with it on exactly as with it off, and have a setting of their own
 * (cimbar_hip_set_stream_colour_vote). Takes effect for combined batches issued after the call. get: writes 1 or 0 to *on and returns 0. */
int cimbar_hip_set_group_colour_vote(cimbar_hip_ctx* ctx, int on);
int cimbar_hip_get_group_colour_vote(cimbar_hip_ctx* ctx, int* on);

/* Multi-capture decoding across calls. A live receiver hands over one capture per call, or a few; these calls keep the group that is still
 * open at the end of a call on the device (at most max_group - 1 members, copies the context owns, about 0.2 MB each) and go on with it in
 * the next stream call. Take a sequence of stream calls on one context whose last call has flush != 0: the groups they report, in order, are
 * the groups ONE cimbar_hip_decode_batch_combined (or _scan_extract_decode_batch_combined_fmt) call reports for the concatenation of their
 * captures with groups_in == NULL and the same settings -- members, gchunks, gmask, erasure retry and all. Each group is reported by the call
 * in which it closes. chunks / masks / status and the colour-correction carry are the plain call's for the same input.
 *   a group closes  when a capture starts a new one (agree(k-1, k) * 1000 < min_agree_permille * cells), when it reaches max_group members (at
 *                   once, in the call of that member), when an unusable capture follows it (capture path), or when flush != 0
 *   groups_out      n ints (may be NULL), the call's own captures: the call-local id of the capture's group if it closes in this call (0, 1, ...
 *                   in closing order = capture order), CIMBAR_HIP_GROUP_OPEN if it stays open, -1 if the capture is unusable
 *   gchunks / gmasks / gsizes  n + 1 slots (capture 0 can close the carried group, every capture can close a group of its own, the flush closes
 *                   the last); slots at or above the closed count are zero. gsizes[g] = the members of group g, those of earlier calls
 *                   included (may be NULL)
 *   n_groups        the groups closed by this call (may be NULL); host outputs: also the return value
 *   n == 0          allowed with flush != 0 (closes and reports the open group; with nothing open: 0 groups; no image argument is read);
 *                   without a flush CIMBAR_HIP_EINVAL
 *   min_agree_permille / max_group  resolved as above and fixed by the first stream call after create or cimbar_hip_combine_stream_reset: a call that
 *                   resolves to other values is CIMBAR_HIP_EINVAL, checked before anything is enqueued. should_preprocess, color_correction, n
 *                   and the capture size may change from call to call. There is no groups_in.
 * Device outputs: the call enqueues and returns 0; whether a group is open, its members and their slots are decided on the device, nothing
 * is read back. Other calls on the context may run between two stream calls (cimbar_hip_decode_batch, the plain combined calls, delivery, the
 * pipelined entry): the stream neither sees their captures nor is disturbed by them. Consecutive stream calls are ordered against each other,
 * whatever their hip_stream. The group taps after a stream call describe the groups it closed.
 * cimbar_hip_combine_stream_reset waits for the stream calls issued so far, drops the open group and forgets the fixed parameters. */
enum { CIMBAR_HIP_GROUP_OPEN = -2 };
int64_t cimbar_hip_decode_batch_combined_stream(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                                int min_agree_permille, int max_group, int flush, uint8_t* chunks, uint32_t* masks, int* groups_out,
                                                uint8_t* gchunks, uint32_t* gmasks, int* gsizes, int* n_groups, int out_mem, void* hip_stream);
int64_t cimbar_hip_scan_extract_decode_batch_combined_stream_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format,
                                                                 int n, int img_mem, int preprocess, int color_correction, int min_agree_permille,
                                                                 int max_group, int flush, uint8_t* chunks, uint32_t* masks, int* status,
                                                                 int* groups_out, uint8_t* gchunks, uint32_t* gmasks, int* gsizes, int* n_groups,
                                                                 int out_mem, void* hip_stream);
int cimbar_hip_combine_stream_reset(cimbar_hip_ctx* ctx);

/* Colour vote in the stream calls (off after cimbar_hip_create; governs the stream calls only, as cimbar_hip_set_group_colour_vote governs the
 * plain combined calls only). With it on, a sequence of stream calls whose last call has flush != 0 reports the group outputs -- gchunks,
 * gmasks, gsizes, the colour of the combined cells and the group colour margin -- that ONE cimbar_hip_decode_batch_combined call with
 * cimbar_hip_set_group_colour_vote(ctx, 1) reports for the concatenation of the captures, byte for byte, each group in the call in which it
 * closes; with cimbar_hip_set_colour_erasure_decode on in both, the group colour retry included. A member's weight w_c = marg_c + 1 depends on
 * the member alone, so the carry holds, per member, the weight of every cell (cells u32, about 50 KB in mode 68; allocated by the first stream
 * call with the setting on) -- no means, matrices or frames.
 * A stream samples the setting in its first call after create or cimbar_hip_combine_stream_reset and holds it, like min_agree_permille and
 * max_group: a stream call that finds it changed is CIMBAR_HIP_EINVAL, checked before anything is enqueued, and leaves the open group as it
 * was. Modes 4 and 8 refuse on != 0 (EINVAL). get: writes 1 or 0 to *on and returns 0. */
int cimbar_hip_set_stream_colour_vote(cimbar_hip_ctx* ctx, int on);
int cimbar_hip_get_stream_colour_vote(cimbar_hip_ctx* ctx, int* on);

/* Torn-capture stitching. A camera's rolling shutter that crosses a display refresh shows frame A on one side of a line and frame B on the
 * other; the next capture shows B, then C. The Reed-Solomon stream is interleaved over the two halves of the frame, so a torn capture alone
 * delivers at most the chunks of the half its tear does not cross, while two consecutive torn captures together hold every cell of the frame
 * they share. These calls decode a batch capture by capture exactly as cimbar_hip_decode_batch / cimbar_hip_scan_extract_decode_batch_fmt do
 * (chunks, masks, status and the colour-correction carry equal theirs for the same input and settings), then, for every pair of consecutive
 * captures k and k+1 of the batch:
 *   lines      axis 0 (a horizontal tear): line(i) = cell i's grid row (y_i - offset) / 9, L = the grid's rows. axis 1 (the tear a phone
 *              held at a right angle to the screen produces): line(i) = its grid column (x_i - offset) / 9, L = the grid's columns.
 *              width(l) = the cells on line l, fewer on the lines that cross the anchors.
 *   eq(i)      symbol and colour both equal in the two captures (the comparison of the group decode's agree(k, k+1))
 *   flag(l)    cnt(l) * 1000 >= min_agree_permille * width(l), cnt(l) = the sum of eq over line l; min_agree_permille <= 0: 750
 *   band       a = the lowest flagged line, b = the highest flagged line + 1, f = the flagged lines
 *   candidate  both captures usable (capture path: extracted), f >= 1, b - a >= min_band (min_band <= 0: 2), 4 f >= 3 (b - a) -- a few
 *              damaged lines inside the band are tolerated -- and a > 0 or b < L: a band over the whole frame means the two captures show one
 *              frame, which is the group decode's case
 *   split      s = (a + b) >> 1, the line farthest from both tears. Direction 0: cell i is capture k+1's if line(i) < s, else capture k's --
 *              the later capture's low lines and the earlier capture's high lines show the shared frame. Direction 1 is the reverse, for a
 *              sensor read the other way round. Symbol and colour are taken from the chosen capture as it decided them.
 *   decode     both directions' cells go through the same Reed-Solomon decode and chunk bookkeeping as one frame (modes 4 / 8: the coupled
 *              stream). No colour-correction matrix is derived, read or carried; nothing is voted, retried (the erasure settings reach
 *              this decode only through cimbar_hip_set_stitch_erasure, below) or filled in from the two captures, which show other frames.
 *   schunks / smasks  2 (n - 1) slots of cimbar_hip_ctx_bufsize bytes / one mask word; pair k, direction d is slot 2k + d. smask is the
 *              stitched decode's own mask, chunks outside it are zero, and so is everything of a pair that is no candidate. The wrong
 *              direction yields chunks of a neighbouring frame or nothing: every chunk in any mask is a genuine chunk, and a sink
 *              (cimbar_hip_deliver_chunks takes the same layout) drops the duplicates.
 *   tears      (n - 1) x 4 int32 {a, b, s, f}, a = b = s = -1 for a pair that is no candidate; may be NULL
 * Every output follows out_mem. Host outputs: synchronises and returns the number of candidate pairs. Device outputs: enqueues only, behind
 * the per-capture decode on the same stream, and returns 0. n == 1: no pair, nothing stitched, returns 0. axis outside {0, 1}, min_band > L
 * or a null required pointer: CIMBAR_HIP_EINVAL, checked before anything is enqueued. Pairs do not span two calls (the stream forms below
 * carry the last capture). Buffers, stream and errors otherwise as for cimbar_hip_decode_batch; no other call's behaviour depends on these. */
int64_t cimbar_hip_decode_batch_stitched(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                         int axis, int min_agree_permille, int min_band, uint8_t* chunks, uint32_t* masks, uint8_t* schunks,
                                         uint32_t* smasks, int32_t* tears, int out_mem, void* hip_stream);
int64_t cimbar_hip_scan_extract_decode_batch_stitched_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n,
                                                          int img_mem, int preprocess, int color_correction, int axis, int min_agree_permille,
                                                          int min_band, uint8_t* chunks, uint32_t* masks, int* status, uint8_t* schunks,
                                                          uint32_t* smasks, int32_t* tears, int out_mem, void* hip_stream);

/* Torn-capture stitching across calls. A live receiver hands over one capture per call, or a few, and a tear's two captures then arrive in two
 * calls; these calls keep a copy of the last capture's decided cells on the device (symbols and colours, one byte per cell each, and one word
 * saying whether the capture is usable) and hold the next stream call's first capture against it. Take a sequence of stitched-stream calls on
 * one context that starts after cimbar_hip_create or cimbar_hip_stitch_stream_reset and uses one axis, min_agree_permille and min_band: it
 * reports, in order, the pairs ONE cimbar_hip_decode_batch_stitched (or _scan_extract_decode_batch_stitched_fmt) call reports for the
 * concatenation of the captures -- tears, schunks and smasks -- each pair in the call that holds its second capture. A pair closes with its
 * second capture, so nothing is ever open and there is no flush.
 *   rows       a call of n captures reports n pair rows: row 0 = (the carried capture, capture 0), row r = (capture r - 1, capture r); row r,
 *              direction d is slot 2r + d. schunks: 2n slots of cimbar_hip_ctx_bufsize bytes, smasks: 2n words, tears: n x 4 int32 (may be NULL)
 *   row 0 without a usable carry  (the first call after create or reset; capture path: the carried capture's extraction failed) is no
 *              candidate: tears {-1, -1, -1, 0}, both slots zero, both masks 0
 *   the rule   otherwise the one above, word for word: eq, flag, band, candidate, split, both directions, the decode and what smask means. No
 *              matrix is derived, read or carried; no vote, no erasure retry (cimbar_hip_set_stitch_erasure does not reach these calls)
 *   chunks / masks / status and the colour-correction carry are the plain call's for the same input
 *   axis, min_agree_permille, min_band, should_preprocess, color_correction, n and the capture size may change from call to call: row 0 is
 *              judged with the parameters of the call that reports it. Only the carry is state
 * n <= 0, a null required pointer, axis outside {0, 1} or min_band > L: CIMBAR_HIP_EINVAL, checked before anything is enqueued, the carry left
 * as it was. Host outputs: synchronises and returns the candidate rows of this call. Device outputs: enqueues only and returns 0; whether row 0
 * has a usable partner is decided on the device from the carried word, nothing is read back. Other calls on the context may run between two
 * stitched-stream calls (cimbar_hip_decode_batch, the plain stitched calls, the combined and combined-stream calls, delivery, the pipelined
 * entry): they neither see nor disturb the carry. Consecutive stitched-stream calls are ordered against each other, whatever their hip_stream.
 * The scratch of the stitched decode is shared with the plain stitched calls: a plain and a stream stitched call running at the same time on
 * two streams are the caller's to order. The stitch taps after a stream call describe its n rows.
 * cimbar_hip_stitch_stream_reset waits for the stitched-stream calls issued so far and forgets the carry. */
int64_t cimbar_hip_decode_batch_stitched_stream(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                                int axis, int min_agree_permille, int min_band, uint8_t* chunks, uint32_t* masks, uint8_t* schunks,
                                                uint32_t* smasks, int32_t* tears, int out_mem, void* hip_stream);
int64_t cimbar_hip_scan_extract_decode_batch_stitched_stream_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format,
                                                                 int n, int img_mem, int preprocess, int color_correction, int axis,
                                                                 int min_agree_permille, int min_band, uint8_t* chunks, uint32_t* masks, int* status,
                                                                 uint8_t* schunks, uint32_t* smasks, int32_t* tears, int out_mem, void* hip_stream);
int cimbar_hip_stitch_stream_reset(cimbar_hip_ctx* ctx);

/* Torn-capture stitching strip by strip (1 after cimbar_hip_create: the rule above, bit for bit). A tear is a straight line on the sensor, so
 * a receiver's roll and perspective put it on a slant in the deskewed frame. When the tear rises over m grid lines across the frame and the
 * two tears lie g lines apart, no whole line reaches 750 once g falls below about 0.75 m, although every column still has g clean shared
 * lines. With strips = S in 2..8 the frame is cut across the lines into S strips and the band is found in each. lines, L, eq,
 * min_agree_permille and min_band are the ones above; for captures k, k+1 and the call's axis:
 *   strip      across(i) = cell i's index on the other axis: axis 0 its grid column (x_i - offset) / 9 with A = the grid's columns, axis 1
 *              its grid row with A = the grid's rows. strip(i) = across(i) * S / A in integers.
 *   width(l, j) the cells of line l in strip j (positive for S <= 8 in every mode; checked once at cimbar_hip_create)
 *   flag(l, j) cnt(l, j) * 1000 >= min_agree_permille * width(l, j), cnt(l, j) = the sum of eq over those cells
 *   per strip  a_j = the lowest flagged line, b_j = the highest flagged line + 1, f_j = the flagged lines. Strip j is located iff f_j >= 1,
 *              b_j - a_j >= min_band and 4 f_j >= 3 (b_j - a_j); its own split is (a_j + b_j) >> 1.
 *   candidate  both captures usable, 2 * located >= S, and some located strip with a_j > 0 or b_j < L (every located strip spanning the whole
 *              frame is the group decode's case, as above)
 *   splits     a located strip keeps its own split as s_j; any other takes the split of the nearest located strip by index, the lower index
 *              on a tie
 *   cells      direction 0: cell i is capture k+1's if line(i) < s_strip(i), else capture k's; direction 1 the reverse
 *   tears      {min a_j, max b_j over the located strips, s_(S >> 1), the sum of f_j over all strips}; no candidate: {-1, -1, -1, that sum}
 * Slots, the decode, smask, zeroes for a pair that is no candidate and the return values are unchanged; host outputs still return the records
 * with a >= 0. The four stitched entry points read the setting when they are called, so it may change between the calls of a stream: row 0
 * is judged with the setting of the call that reports it, like axis. set: strips outside 1..8 is CIMBAR_HIP_EINVAL and changes nothing;
 * every mode accepts 1..8. get: writes the setting to *strips and returns 0. For a hand-held receiver 4 to 8 is the advice. */
int cimbar_hip_set_stitch_strips(cimbar_hip_ctx* ctx, int strips);
int cimbar_hip_get_stitch_strips(cimbar_hip_ctx* ctx, int* strips);

/* Erasure retry in the stitched decode (off after cimbar_hip_create: everything above, byte for byte; nothing more is launched, allocated or
 * written). A stitched frame is built from the worse-exposed edges of two captures, so a block that fails errors-only decoding by a few bytes
 * is its usual failure. With the setting on, slot 2k + d of cimbar_hip_decode_batch_stitched / _scan_extract_decode_batch_stitched_fmt (host or
 * device outputs, either axis, strips 1..8) is retried after the decode above:
 *   source     cell i of the slot came from capture src(i), k or k + 1: the selection of "split" above (with strips, of "cells")
 *   d_sym(i)   the symbol confidence of cimbar_hip_set_erasure_decode, evaluated in capture src(i): the popcount of the 8x8 hash of that
 *              capture's bit plane at the cell's final position XOR the tile hash of the stitched symbol; the final position is the grid
 *              position plus that capture's drift where that capture took a flood pass, the grid position otherwise
 *   symbol retry  with cimbar_hip_set_erasure_decode on (its sym_distance and max_erasures), for a live slot whose smask lacks symbol chunks:
 *              the blocks of the missing symbol chunks, a byte's score = max over its two cells of d_sym - sym_distance + 1
 *   margin(i)  the colour confidence of cimbar_hip_set_colour_erasure_decode in capture src(i): second-smallest minus smallest squared
 *              distance of the classifier, on that capture's cell mean where it took no flood pass, on the 6x6 mean at the drifted position
 *              where it did, under the matrix that capture's colours were decided with (active flag included)
 *   colour retry  with cimbar_hip_set_colour_erasure_decode on (its colour_margin and max_erasures), behind the symbol retry, for a live slot
 *              whose smask lacks colour chunks: score = colour_margin - margin, max over a byte's four cells
 *   unchanged  selection (the max_erasures highest scores, ties to the lower byte), acceptance (the codeword check, nothing located in the
 *              padding, 2 errors <= parity - erasures - 6), a failed block with nothing flagged is not retried, a block errors-only decoding
 *              accepted is decoded again with no erasure; a chunk whose blocks are all accepted joins smask with its bytes, the slots of
 *              chunks still missing stay zero
 *   never touched  chunks already in smask, the tear records, the line counts, the stitched cells (CIMBAR_HIP_TAP_STITCH_CELLS), the block
 *              flags, the per-capture chunks / masks / status and the colour-correction carry
 * smask with the setting on is always a superset of smask with it off. A slot that is not live, or whose chunks are complete, is left at its
 * first test. With neither erasure setting on nothing runs. The stitched-stream calls behave with the setting on exactly as with it off: their
 * carry holds cells, not bit planes or cell means (carrying confidences is a later change). The stitched calls read the setting when they are
 * called. Modes 4 and 8 (one coupled stream): on != 0 is CIMBAR_HIP_EINVAL. get: writes the setting to *on and returns 0. */
int cimbar_hip_set_stitch_erasure(cimbar_hip_ctx* ctx, int on);
int cimbar_hip_get_stitch_erasure(cimbar_hip_ctx* ctx, int* on);

/* ---- repeat-capture skipping: one decode per displayed frame ------------------------------------------------------------------------------
 * A camera films the display faster than it changes, so every frame arrives as a run of two to four near-identical captures, and the calls
 * above decode each of them in full. These two calls find the runs IN FRONT of the decode, decode one capture of each run, and decode the
 * others only where that one came back incomplete. Opt-in; no other call's behaviour depends on them. Modes 68 / 67 / 66 (the signature was
 * checked on their palette: four ink colours on black); modes 4 and 8: CIMBAR_HIP_EINVAL.
 *   signature  cell c of a usable capture's deskewed frame, nominal top-left (x, y) (no drift): R_c, G_c, B_c = the channel sums over pixel
 *              rows y + 2 .. y + 5 and columns x .. x + 7, S_c = R_c + G_c + B_c; R_A, B_A, S_A = the sums of R_c, B_c, S_c over the frame's
 *              cells; sig_c = [R_c S_A > S_c R_A] | [B_c S_A > S_c B_A] << 1. Strict comparisons, unsigned 64-bit arithmetic. The frame is
 *              read as handed in, or as the warp wrote it; sharpening plays no part. (CIMBAR_HIP_TAP_REPEAT_SIG)
 *   agreement  agree(k, k + 1) = the cells with equal sig (CIMBAR_HIP_TAP_REPEAT_AGREE)
 *   runs       capture k starts a new run when it is the first; when agree(k - 1, k) * 1000 < min_agree_permille * cells (<= 0: 900; above
 *              1000: CIMBAR_HIP_EINVAL); when the run before it already has max_run members (<= 0: 4; above 8: CIMBAR_HIP_EINVAL); or
 *              when capture k - 1 or k is unusable (capture path only: its extraction failed). An unusable capture is in no run: runs_out
 *              and roles -1, mask 0, zeroed slot, as in the plain call. Runs are numbered from 0 in capture order and do not span calls.
 *   representative  member (len - 1) / 2 of a run: the first of two, the second of three or four. The reasoning -- on an LCD the first capture
 *              after a switch tends to ghost and the last may catch the next switch -- is a guess; nobody has measured it.
 *   pass 1     the representatives are decoded in capture order, exactly as one plain call would decode them
 *   pass 2     the other members of every run whose representative's mask is not full are decoded in capture order, again exactly as one
 *              plain call; if there are none, no second pass runs
 *   roles      per capture: CIMBAR_HIP_ONCE_REPRESENTATIVE (1), _FALLBACK (2: decoded in pass 2), _SKIPPED (0), _UNUSABLE (-1)
 *   chunks / masks  of a decoded capture: what the plain call delivers for it, bit for bit; of a skipped one: mask 0 and a zeroed slot.
 *              Capture path: status is the plain call's for every capture -- extraction runs for all of them
 *   contract   list 1 = the representatives, list 2 = the pass-2 members. The per-capture results of list 1, then of list 2, are the
 *              results of two consecutive plain calls -- cimbar_hip_decode_batch on those frames, resp.
 *              cimbar_hip_scan_extract_decode_batch_fmt on those captures -- on a context in the same state: the colour-correction carry
 *              (cimbar_hip_get_ccm afterwards) and the erasure, colour-erasure and relaxed-flood settings in force included
 *   per run    n slots, zero at and above the run count: rmasks[r] = the OR of the members' masks; rchunks[r] chunk j from the representative
 *              where it delivered it, else from the lowest-index member that did, else zeros; *n_runs = the run count. One run is one
 *              displayed frame: this is the row to hand to cimbar_hip_deliver_chunks
 *   runs_out, roles, rchunks, rmasks, n_runs  may each be NULL. Every output follows out_mem.
 *   synchronisation  the host needs the length of list 1, and then of list 2, to size the decode launches: each call reads a 4-byte count
 *              back after the run walk and (unless every capture is its own run) again after pass 1 -- at most two stream synchronisations
 *              in the middle of the call, device outputs included. After that a device-output call enqueues the rest and returns 0; a
 *              host-output call synchronises and returns the run count. This is the one place where these calls differ from "only enqueues".
 *   known limit  two different frames whose colour streams are equal are taken for repeats, and the second is dropped (an uncompressed file
 *              of constant bytes can do that). A fountain receiver survives a dropped frame; a caller who cannot accept the limit uses the
 *              plain or the combined calls.
 * Buffers, stream and errors otherwise as for cimbar_hip_decode_batch / cimbar_hip_scan_extract_decode_batch_fmt; a null chunks or masks,
 * n <= 0 or a parameter out of range is CIMBAR_HIP_EINVAL, checked before anything is enqueued. Runs across calls: the _once_stream calls
 * below. A run that stays incomplete after pass 2 is given up here; cimbar_hip_set_once_rescue (below) decodes it once more from all its
 * members' cells, as the combined calls decode a group. A torn capture between two runs is a run of one and is decoded in pass 1;
 * cimbar_hip_set_once_tear_skip (below) leaves it undecoded where both neighbour runs are complete. Not covered: the pipelined and
 * frame-async entry points, the combined calls' colour vote and stream forms, stitching a frame out of torn captures (the stitched calls),
 * the undistort path and the auto-detection objects. */
enum {
	CIMBAR_HIP_ONCE_UNUSABLE = -1,
	CIMBAR_HIP_ONCE_SKIPPED = 0,
	CIMBAR_HIP_ONCE_REPRESENTATIVE = 1,
	CIMBAR_HIP_ONCE_FALLBACK = 2,
	CIMBAR_HIP_ONCE_TORN = 3        /* only with cimbar_hip_set_once_tear_skip on: a torn boundary capture that was left undecoded */
};
int64_t cimbar_hip_decode_batch_once(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                     int min_agree_permille, int max_run, uint8_t* chunks, uint32_t* masks, int* runs_out, int* roles,
                                     uint8_t* rchunks, uint32_t* rmasks, int* n_runs, int out_mem, void* hip_stream);
int64_t cimbar_hip_scan_extract_decode_batch_once_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n,
                                                      int img_mem, int preprocess, int color_correction, int min_agree_permille, int max_run,
                                                      uint8_t* chunks, uint32_t* masks, int* status, int* runs_out, int* roles, uint8_t* rchunks,
                                                      uint32_t* rmasks, int* n_runs, int out_mem, void* hip_stream);

/* Run rescue (off after cimbar_hip_create): a third pass of the two once-calls above, over exactly the runs the first two leave incomplete.
 * The combined calls deliver a frame whose captures are each damaged somewhere else, at the price of decoding every capture; the once-calls
 * decode one capture per run but only OR the members' masks. With the setting on, and at least one of rchunks / rmasks not NULL, after pass 2:
 *   tried      a run is tried when it has at least two members, all of them decoded, and the OR of their masks is not full. All members are
 *              decoded exactly when the representative's mask was not full (pass 2 then took the rest). A run of one is never tried, nor
 *              a run whose representative or whose pass-2 members completed it. No tried run in a call: the rescue launches no decode.
 *   group      a tried run's members, in capture order, are one group of cimbar_hip_decode_batch_combined: the combined cells are its
 *              -- per cell the symbol vote over 2 d_c(t) - [t == s_c] and the colour plurality with its two tie-breaks -- taken from each
 *              member's bit plane, symbols, colours, drift and flood flag as the pass that decoded it left them. The representatives'
 *              cells are kept on the device across pass 2 (about 0.18 MB per run that may need them, mode 68). No colour-correction
 *              matrix is derived, read or carried.
 *   decode     Reed-Solomon over the combined cells and the chunk bookkeeping as in the combined call; with
 *              cimbar_hip_set_erasure_decode on, its symbol-erasure retry as well
 *   row        rmasks[r] = the combined decode's mask | the members' masks | the chunks the retry added; rchunks[r] chunk j = the combined
 *              decode's chunk where it delivered it, else that of the lowest-index member that did, else zeros. For a tried run this
 *              replaces the row described under "per run"; the rows of all other runs are that row, byte for byte. rmasks[r] with the
 *              setting on is always a superset of rmasks[r] with it off. For a tried run the row equals gchunks / gmasks of
 *              cimbar_hip_decode_batch_combined (or _scan_extract_decode_batch_combined_fmt) with groups_in = runs_out and the same
 *              settings, provided no capture's decode depends on what was decoded before it (color_correction 0 or 1).
 *              (CIMBAR_HIP_TAP_ONCE_RESCUE, CIMBAR_HIP_TAP_ONCE_RESCUE_CELLS)
 *   unchanged  per-capture chunks / masks / status, runs_out, roles, *n_runs, the return value, the colour-correction carry afterwards and
 *              the two mid-call read-backs: which runs are tried is decided on the device, nothing more is read back. With the setting
 *              off no call launches, allocates or writes anything it did not before.
 * The setting governs cimbar_hip_decode_batch_once and cimbar_hip_scan_extract_decode_batch_once_fmt only: the _once_stream calls below behave
 * with it on exactly as with it off (their carry holds masks and a chunk row, no cells). Modes 4 and 8 refuse on != 0 (EINVAL), as they
 * refuse the once-calls. Takes effect for once-calls issued after the call. The rescue uses the group scratch of the combined calls: a
 * once-call with the setting on and a combined call on the same context at the same time on two streams is the caller's to order, as two
 * combined calls are. get: writes 1 or 0 to *on and returns 0.
 * Not covered: the once-stream calls, the colour vote (cimbar_hip_set_group_colour_vote is not consulted), stitching (but see tear salvage
 * below: a torn capture's good side can join a tried run's vote), the undistort path, the auto-detection objects, the C++ adapter and the
 * receive shim. */
int cimbar_hip_set_once_rescue(cimbar_hip_ctx* ctx, int on);
int cimbar_hip_get_once_rescue(cimbar_hip_ctx* ctx, int* on);

/* Tear skipping (off after cimbar_hip_create): the two once-calls above leave a torn boundary capture undecoded. A camera that films faster
 * than the display changes catches a frame switch in about one capture of four: frame P on one side of a line, frame N on the other. Its
 * signature agrees with each neighbour on about 600 permille of the cells, so it is a run of one, its own representative, and is decoded in
 * pass 1 -- through the flood path, for chunks its neighbour runs already have. With the setting on, runs, runs_out, *n_runs, the return
 * value and the number of mid-call read-backs are what they are with it off; only who is decoded changes:
 *   lines      line(i), L and width(l) are those of the stitched calls: axis 0 the grid rows, axis 1 the grid columns. axis 2 evaluates both:
 *              a capture is torn if either axis says so, and axis 0's tear is reported when both do.
 *   eligible   capture k is eligible when 1 <= k <= n - 2, captures k - 1, k and k + 1 are usable, and k's run has one member
 *   per line   cntP(l) = the cells on line l whose sig equals capture k - 1's, cntN(l) the same against capture k + 1's;
 *              flagP(l) = cntP(l) * 1000 >= line_permille * width(l), flagN(l) likewise; p(l) = flagP & !flagN, q(l) = flagN & !flagP
 *   orientation and split  o = 0: P's frame is on the low lines, (a, b) = (p, q); o = 1: (a, b) = (q, p). For a split s with
 *              min_side <= s <= L - min_side: first = #{l < s : a(l)}, last = #{l >= s : b(l)}; (o, s) is admissible when
 *              8 first >= 7 s and 8 last >= 7 (L - s). The 7/8 per side tolerates the line the tear crosses and a few damaged lines; the
 *              guard below bounds what a wrong "torn" can cost. It is a rule constant, not a measurement.
 *   candidate  an eligible capture with an admissible (o, s). Its tear is the admissible pair with the largest first + last; ties go to
 *              the lower o, then the lower s. (CIMBAR_HIP_TAP_ONCE_TEAR)
 *   pass 1     list 1 = the representatives without the candidates, in capture order
 *   guard      after pass 1, a candidate whose two neighbour runs' representatives both came back with full masks is torn: role
 *              CIMBAR_HIP_ONCE_TORN, mask 0 and a zeroed slot, its run's row zero and rmask 0, never decoded. A neighbour that is itself a
 *              candidate has not come back at all, so of two candidates in a row neither is torn.
 *   pass 2     every other candidate joins list 2 in capture order, with role _FALLBACK, and is decoded there exactly as a plain call
 *              decodes it: wherever a neighbour run is not complete, nothing is withheld that the setting-off call would have decoded
 *   contract   as above: the per-capture results of list 1, then of list 2, are the results of two consecutive plain calls on a context
 *              in the same state
 *   run rescue composes unchanged: a candidate is a run of one and is never tried
 *   synchronisation  as above: the length of list 1, then of list 2, 4 bytes each. The length of list 1 is no longer the run count once
 *              a candidate exists; a host-output call takes the run count from its last copy. Nothing further is read back. With the
 *              setting off no call launches, allocates or writes anything it did not before.
 * set: axis -1 = off (the other two arguments are then not looked at; get reports -1, 750, 2), 0, 1 or 2; anything else is
 * CIMBAR_HIP_EINVAL. line_permille <= 0 resolves to 750, above 1000 is CIMBAR_HIP_EINVAL. min_side <= 0 resolves to 2; 2 * min_side > L of
 * the mode on the chosen axis (axis 2: on either) is CIMBAR_HIP_EINVAL. A refused call changes nothing. get reports the resolved values (each
 * pointer may be NULL). Modes 4 and 8 refuse any axis other than -1 (EINVAL), as they refuse the once-calls. Takes effect for once-calls
 * issued after the call. The once-stream calls behave with the setting on exactly as with it off: a torn capture's successor is not known
 * when its call has to decide.
 * Not covered: the once-stream calls; slanted tears (the strip-by-strip form); two torn captures in a row, which agree with each other, form
 * a run of two and are decoded as before; the undistort path, the auto-detection objects, the C++ adapter and the receive shim. Using a
 * torn capture's good side when a neighbour run is incomplete is tear salvage, below. */
int cimbar_hip_set_once_tear_skip(cimbar_hip_ctx* ctx, int axis, int line_permille, int min_side);
int cimbar_hip_get_once_tear_skip(cimbar_hip_ctx* ctx, int* axis, int* line_permille, int* min_side);

/* Tear salvage (off after cimbar_hip_create): a torn capture's sides join the run rescue of its neighbour runs. A candidate of tear skipping
 * that stands beside an incomplete run is decoded whole in pass 2. It is half frame P and half frame N, so it delivers next to nothing, but
 * on every line on P's side of the tear its cells are correctly decoded cells of P, and likewise for N. With the setting EFFECTIVE those
 * cells vote in the group decode of the neighbour run. The setting is effective in a plain once-call only when all three hold: run rescue
 * is on, tear skipping's axis is not -1, and rchunks or rmasks is asked for. Otherwise the call behaves, byte for byte and launch for
 * launch, as with the setting off. Everything below applies after pass 2, with the setting effective:
 *   sides      a candidate k has the record {w, s, first, last} (CIMBAR_HIP_TAP_ONCE_TEAR), axis = w >> 1, o = w & 1, and L lines on that
 *              axis. With the guard g: low = [0, s - g) and high = [s + g, L). Its P side is low when o = 0 and high when o = 1; its N side
 *              is the other one. The P side is the side on which the candidate agreed with capture k - 1, the N side the one on which it
 *              agreed with capture k + 1. A side whose range is empty gives no partial.
 *   partials   let run r be a run that is no candidate's run, with first member f and last member e. Its following partial is capture
 *              e + 1, if that capture is a candidate with role _FALLBACK, taken with its P side. Its preceding partial is capture f - 1, if
 *              that capture is such a candidate, taken with its N side. A candidate beside a run whose representative is incomplete is
 *              always in list 2, by tear skipping's guard. One candidate can serve both of its neighbours. A candidate's own run is never
 *              tried, as before.
 *   qualifies  (decided in front of pass 2, when the representative's cells must be kept) the representative's mask is not full, and the
 *              run has at least two members or at least one partial
 *   tried      the run qualifies, and the OR of the full members' masks after pass 2 is not full. A run that qualifies only through its
 *              partial is a run of one: it has no pass-2 member, so all its members are decoded.
 *   group order  the full members first, in capture order; then the preceding partial, then the following partial. A partial joins only
 *              while the group has fewer than 8 members. "Lowest member index" in the combined cells' tie-breaks means the position in this
 *              order. Member 0 is always a full member.
 *   participation  a full member takes part in every cell. A partial takes part in cell i if and only if lo <= line_axis(i) < hi, with
 *              line_axis(i) the stitched calls' line of cell i on the partial's axis.
 *   combined cells  the rule of the combined calls, unchanged, but per cell over that cell's participants: the symbol vote over
 *              2 d_c(t) - [t == s_c], the colour plurality with its two tie-breaks, and the margin. A cell with one participant takes that
 *              participant's symbol and colour, and its symbol counts as undisputed. A group counts as disputed where the participants of
 *              any cell differ.
 *   decode and row  as the run rescue: Reed-Solomon over the combined cells, the chunk bookkeeping, and the symbol-erasure retry when it
 *              is on. Only the FULL members' masks and chunks enter the row; a partial contributes cells and nothing else, because its own
 *              decode can hold chunks of the other frame when the tear is near an edge, and those must never reach this run's row.
 *              rmasks[r] is a superset of the OR of the full members' masks. For a run the rescue alone would also try, NO superset of
 *              the rescue-alone row is promised: the partial's cells change the vote, and a vote can lose a chunk as well as gain one.
 *              CIMBAR_HIP_TAP_ONCE_RESCUE and _RESCUE_CELLS keep their meaning; their "members" are the full members.
 *              (CIMBAR_HIP_TAP_ONCE_SALVAGE)
 *   unchanged  per-capture chunks, masks and status; runs_out, roles and *n_runs; the return value and the colour-correction carry; the
 *              rows of every run that is not tried; the two 4-byte read-backs, with nothing further read back. The rescue's store and
 *              scratch are sized for min(|list 1|, 2 |list 2|) runs instead of min(|list 1|, |list 2|). With the setting off no call
 *              launches, allocates or writes anything it did not before.
 * set: guard_lines -1 resolves to 1; 0 .. 16 are legal; anything else is CIMBAR_HIP_EINVAL. Modes 4 and 8 refuse on != 0 (EINVAL). A refused
 * call changes nothing. get reports the resolved values (each pointer may be NULL). Takes effect for once-calls issued after the call. The
 * once-stream calls ignore the setting.
 * Not covered: the once-stream calls; slanted tears (the strip-by-strip form); two torn captures in a row; the colour vote in the salvage
 * group; the undistort path, the auto-detection objects, the C++ adapter and the receive shim. */
int cimbar_hip_set_once_tear_salvage(cimbar_hip_ctx* ctx, int on, int guard_lines);
int cimbar_hip_get_once_tear_salvage(cimbar_hip_ctx* ctx, int* on, int* guard_lines);

/* ---- repeat-capture skipping across calls: the open run is carried from call to call -------------------------------------------------------
 * A live receiver hands over one capture (or a few) per call, so a run of repeats spans calls. The two _once_stream calls are the calls above
 * with one piece of state on the device: what the previous once-stream call on this context left. Signature, agree, min_agree_permille,
 * max_run, roles and usability are exactly those of the plain once-calls; modes 4 and 8: CIMBAR_HIP_EINVAL.
 *   carry      the signature of the previous call's last capture; one word saying whether that capture was usable; and, if it was, the open
 *              run it belongs to: len = its members so far, over all calls; P = the OR of the masks its decoded members delivered; its chunk
 *              row, filled as rchunks is. After cimbar_hip_create or cimbar_hip_once_stream_reset nothing is carried. The carry sits in two
 *              slots used in turn: a call reads one and writes the other, and they change roles only when the call returns its result, so a
 *              call that returns an error leaves the carry as it was. (CIMBAR_HIP_TAP_REPEAT_CARRY)
 *   walk       capture k continues the run of its predecessor (k = 0: the carried capture's run) if and only if both are usable,
 *              agree * 1000 >= min_agree_permille * cells, and that run has fewer than max_run members, counting those of earlier calls.
 *              Otherwise a usable capture starts a run and an unusable one is in no run. Runs are numbered from 0 in the call's capture
 *              order; *continued = 1 if run 0 continues the carried run, else 0. Over any split of a capture sequence into calls the run
 *              boundaries are those ONE plain once-call reports for the concatenation with the same two parameters.
 *   segment    a run's members in this call. P of the continued run's segment is the carried mask, P of every other segment is 0. The
 *              representative of a segment is its member (seg_len - 1) / 2.
 *   pass 1     for every segment whose P is not full: its representative, in capture order. A segment whose P is full decodes nothing: all
 *              its members are CIMBAR_HIP_ONCE_SKIPPED.
 *   pass 2     for every segment with P | (its representative's mask) not full: its other members, in capture order; none: no second pass
 *   contract   as above: the per-capture results of list 1, then of list 2, are the results of two consecutive plain calls on a context in
 *              the same state; a skipped or unusable capture has mask 0 and a zeroed slot; capture path: extraction runs for every capture
 *              and status is the plain call's
 *   per run    n slots, zero at and above the run count: rmasks[r] = P | the OR of the members' masks; rchunks[r] chunk j from the carried row
 *              where P has bit j, else from the representative where it delivered it, else from the lowest-index member that did, else
 *              zeros. The row is cumulative over the run's calls: handed to cimbar_hip_deliver_chunks with CIMBAR_HIP_DELIVER_DEDUP and
 *              _REMEMBER, each chunk reaches the sink once.
 *   new carry  the call's last capture: its signature and its usable word; if it is usable, its run: len = (the carried len if the run is the
 *              continued one, else 0) + seg_len, P = rmasks of that run, the row = rchunks of that run
 *   no flush   a run is reported in every call it has members in, so nothing is ever open from the caller's side
 *   parameters min_agree_permille, max_run, should_preprocess / preprocess, color_correction, n and the capture size may change from call to
 *              call: capture 0 is judged with the parameters of the call that holds it
 *   one call   directly after create or reset reports, in every output, what the plain once-call reports for the same input; *continued = 0
 *   synchronisation  as above: the length of list 1 is read back after the walk and, if list 1 is neither empty nor all n captures, the
 *              length of list 2 after pass 1. A call whose list 1 is empty enqueues no decode at all.
 *   ordering   consecutive once-stream calls are ordered against each other whatever their hip_stream. Other calls on the context neither
 *              see nor disturb the carry, but the scratch of the run search is shared with the plain once-calls: running one of each at the
 *              same time on two streams is the caller's to order.
 *   continued  may be NULL; it follows out_mem. Everything else as for the plain once-calls, the known limit included. Arguments are checked
 *              before anything is enqueued.
 * cimbar_hip_once_stream_reset waits for the once-stream calls issued so far and forgets the carry.
 * Not covered: the pipelined and frame-async entry points, composing with the combined / stitched calls, the undistort path, the
 * auto-detection objects, a variant without read-backs. */
int64_t cimbar_hip_decode_batch_once_stream(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                            int min_agree_permille, int max_run, uint8_t* chunks, uint32_t* masks, int* runs_out, int* roles,
                                            uint8_t* rchunks, uint32_t* rmasks, int* n_runs, int* continued, int out_mem, void* hip_stream);
int64_t cimbar_hip_scan_extract_decode_batch_once_stream_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n,
                                                             int img_mem, int preprocess, int color_correction, int min_agree_permille, int max_run,
                                                             uint8_t* chunks, uint32_t* masks, int* status, int* runs_out, int* roles,
                                                             uint8_t* rchunks, uint32_t* rmasks, int* n_runs, int* continued, int out_mem,
                                                             void* hip_stream);
int cimbar_hip_once_stream_reset(cimbar_hip_ctx* ctx);

/* ---- chunk delivery: a batch's slots and masks -> what a fountain sink eats --------------------------------------------------------------
 * The batch entry points above report a frame's chunks in fixed slots plus one mask word. The reference's receive interface has another shape:
 * cimbard_scan_extract_decode returns the delivered chunks packed front to back (escrow_buffer_writer), and cimbard_fountain_decode(buf, size)
 * walks such a buffer and hands fountain_decoder_sink::decode_frame one chunk at a time. cimbar_hip_deliver_chunks is that step for a whole batch,
 * on the device, and can leave out what the sink would refuse anyway.
 *   chunks / masks : n frames as any batch entry point writes them -- n * cimbar_hip_ctx_bufsize(ctx) bytes and n words (the gchunks / gmasks of
 *                    a combined call have the same layout); in_mem says where they lie
 *   candidates     : the (frame, slot) pairs whose mask bit is set, in ascending frame * chunks_per_frame + slot
 *   flags          : 0 keeps every candidate (escrow_buffer_writer per frame, concatenated over the batch), else an OR of
 *     CIMBAR_HIP_DELIVER_DROP_EMPTY  drop candidates whose header says file size 0 -- (b0 & 0x80) == 0 and b1 == b2 == b3 == 0,
 *                                    FountainMetadata::file_size -- which fountain_decoder_sink::decode_frame refuses (-11): the all-zero chunks
 *                                    of a too-small frame. Applied first: a dropped chunk takes no part in what follows
 *     CIMBAR_HIP_DELIVER_DEDUP       of the candidates whose six header bytes (FountainMetadata::md_size) are equal, keep the first. All 48 bits
 *                                    are compared, never a hash of them; payload bytes play no part (the sink keeps the first one too)
 *     CIMBAR_HIP_DELIVER_REMEMBER    implies DEDUP; also drop candidates whose header an earlier REMEMBER call on this context delivered, and
 *                                    remember the headers this call delivers
 *   packed : the kept chunks back to back, n * cimbar_hip_ctx_bufsize(ctx) bytes of room; src (may be NULL): n * chunks_per_frame words of room,
 *            src[k] = frame * chunks_per_frame + slot of packed chunk k; count: one word. Only packed[0 .. count * chunk_size) and
 *            src[0 .. count) are written. out_mem says where the three lie.
 * Device outputs: the call only enqueues on hip_stream and returns 0. Host outputs: it synchronises and returns count. in_mem and out_mem are
 * independent; NULL hip_stream as for cimbar_hip_decode_batch. n <= 0, a null chunks / masks / packed / count, unknown flag bits, an unknown memory
 * kind or more than 2^24 slots: CIMBAR_HIP_EINVAL, checked before anything is enqueued. cimbard_fountain_decode(packed, count * chunk_size) takes
 * the result in one piece.
 * The call reads no decode state and is ordered against nothing but hip_stream and the context's previous delivery call (they share scratch): after
 * cimbar_hip_decode_batch_pipelined it goes on the caller's stream behind a cimbar_hip_pipeline_wait that covers the batch.
 *
 * REMEMBER keeps the delivered headers in a device-resident open-addressing table of full 48-bit keys that the context owns (allocated by the
 * first REMEMBER call or by cimbar_hip_delivery_reset). Two rules hold:
 *   1. a chunk that is not a duplicate is never dropped. The table is kept at most half full; a call whose new headers would pass that records
 *      NONE of them, still drops what is already remembered, still dedups within itself, and sets the sticky `overflowed` flag: an overflow
 *      lets duplicates through in later calls and loses nothing;
 *   2. packed, src and count are a function of the inputs and the remembered set alone -- the same calls in the same order give the same bytes.
 * cimbar_hip_delivery_reset forgets every header and clears the flag; capacity_log2 0 = the default (20: 2^20 entries, 8 MiB), else 4 .. 24
 * (anything else: CIMBAR_HIP_EINVAL). cimbar_hip_delivery_stats waits for the delivery calls issued so far and reports the headers remembered,
 * the table's entries (0 while there is no table) and the flag; each pointer may be NULL.
 * The auto-detection objects are not covered (their chunk size differs from capture to capture). */
enum {
	CIMBAR_HIP_DELIVER_DEDUP = 1,
	CIMBAR_HIP_DELIVER_REMEMBER = 2,
	CIMBAR_HIP_DELIVER_DROP_EMPTY = 4
};
int64_t cimbar_hip_deliver_chunks(cimbar_hip_ctx* ctx, const uint8_t* chunks, const uint32_t* masks, int n, int in_mem, unsigned flags,
                                  uint8_t* packed, int32_t* src, int32_t* count, int out_mem, void* hip_stream);
int cimbar_hip_delivery_reset(cimbar_hip_ctx* ctx, int capacity_log2);
int cimbar_hip_delivery_stats(cimbar_hip_ctx* ctx, int64_t* remembered, int64_t* capacity, int* overflowed);

/* ---- the encode half ("next" row of the scope table: on-device frame synthesiser) --------------------------------------------
 * Encoder::encode_next (src/lib/encoder/Encoder.h:69-129) for n frames at once: each frame takes 7500 payload bytes (the 60
 * reads of 125 bytes a fountain_encoder_stream / ifstream would have served), RS(155,125)-encodes them (libcorrect encode.c:3-34),
 * stripes the 4 symbol bits and 2 colour bits of every cell through the interleave (CimbWriter.cpp:84-95, Interleave.h:8-24) and
 * pastes tile colour*16+symbol (Common.cpp:150-171) at every cell of a 1024x1024 RGB8 frame.
 * The background / anchors / guides come from a template frame the caller supplies once (an empty CimbWriter image,
 * CimbWriter.cpp:39-77): this library ships no bitmap assets of its own. */
int cimbar_hip_set_template(cimbar_hip_ctx* ctx, const uint8_t* rgb_template, int mem);
int cimbar_hip_encode_batch(cimbar_hip_ctx* ctx, const uint8_t* payload, int n, int payload_mem, uint8_t* rgb_out, int rgb_mem,
                            void* hip_stream);

/* ---- the stage in front of the decoder ("next" row 2 of the scope table: Scanner's image preparation + Deskewer) ----------------------
 * The reference turns a camera capture into the decoder's 1024x1024 frame with Extractor::extract (src/lib/extractor/Extractor.h:29-45):
 * Scanner (gray -> small Gaussian -> Otsu threshold, Scanner.h:148-165; then a sparse scan-line search for the four anchors on that
 * binary image, Scanner.h:277-405) and Deskewer::deskew (cv::getPerspectiveTransform + cv::warpPerspective INTER_LINEAR,
 * Deskewer.h:26-40). These two calls are the image passes on their own (a caller with its own anchor search, or the adapter's
 * cimbar_amd::Deskewer); the whole of Extractor::extract, anchor search included, is cimbar_hip_extract_batch below. The warp's output can
 * stay in device memory for cimbar_hip_decode_batch. Any width x height RGB8 capture (densely packed frames); OpenCV's arithmetic is restated,
 * see DESIGN.md.
 *   cimbar_hip_scan_preprocess : n captures -> n * width * height bytes (0 / 255) = Scanner::preprocess_image(img, fast = true);
 *                                thresholds (n ints, may be NULL) receives the Otsu thresholds. Blur unit as in Scanner.h:157-159 (3x3 below 1500 px on the short side, 5x5 below 2500, 9x9 below 4500, 17x17 below 8500); 8500 px and more: EDIM.
 *   cimbar_hip_deskew_batch    : corners = n * 8 floats in HOST memory, per capture top-left, top-right, bottom-left, bottom-right (x, y)
 *                                exactly as Corners::all() returns them (Corners.h:45-53); frames = n * 1024*1024*3 bytes = what
 *                                Deskewer(0, {1024,1024}, 30).deskew(img, corners) returns.
 * Buffers, stream and errors as for cimbar_hip_decode_batch (host outputs: synchronises; device outputs: enqueues and returns 0). */
int cimbar_hip_scan_preprocess(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int n, int rgb_mem,
                               uint8_t* binary, int* thresholds, int out_mem, void* hip_stream);
int cimbar_hip_deskew_batch(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int n, int rgb_mem,
                            const float* corners, uint8_t* frames, int out_mem, void* hip_stream);

/* Extractor::extract (src/lib/extractor/Extractor.h:29-45) for n captures, entirely on the device: Scanner (image preparation AND the
 * anchor search: Scanner.h:277-405, Scanner.cpp:52-202, ScanState.h:21-104) -> Corners (Corners.h:45-73) -> Deskewer::deskew.
 *   status  : n ints, Extractor::FAILURE 0 / SUCCESS 1 / NEEDS_SHARPEN 2 (Extractor.h:18-20). A capture whose anchor search overflows the fast
 *             kernels' fixed-size work lists (hundreds of anchor-like patterns on one scan line) is searched again serially with lists of
 *             16 384 entries (up to 16 such captures per batch); -1 = those overflowed too, treated as a failure
 *   corners : n * 8 floats, Corners::all() (top-left, top-right, bottom-left, bottom-right; x, y); may be NULL. Unset where status <= 0
 *   frames  : n * 1024*1024*3 bytes, black where status <= 0
 * status / corners / frames share out_mem. Buffers, stream and errors as for cimbar_hip_decode_batch. */
int cimbar_hip_extract_batch(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int n, int rgb_mem, uint8_t* frames,
                             int* status, float* corners, int out_mem, void* hip_stream);

/* cimbard_scan_extract_decode (src/lib/cimbar_js/cimbar_recv_js.cpp:148-189) / the body of cimbar.cpp's decode loop (:124-162) for n
 * captures: extract, then Decoder::decode_fountain on what came out, the deskewed frames never leaving the device.
 *   preprocess : 1 sharpen every frame, 0 none, anything else ("-1 == guess", cimbar.cpp:190) where the extractor said NEEDS_SHARPEN
 *   chunks / masks : as for cimbar_hip_decode_batch; a capture whose extraction failed delivers nothing (mask 0, slots zeroed)
 *   status     : as for cimbar_hip_extract_batch; may be NULL
 * Host outputs: synchronises and returns the total good bytes; device outputs: enqueues and returns 0. */
int64_t cimbar_hip_scan_extract_decode_batch(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int n, int rgb_mem,
                                             int preprocess, int color_correction, uint8_t* chunks, uint32_t* masks, int* status, int out_mem,
                                             void* hip_stream);

/* ---- the capture's pixel format: the `format` argument of the reference's own C ABI for this step ----------------------------------------
 *     int cimbard_scan_extract_decode(const unsigned char* imgdata, unsigned imgw, unsigned imgh, int format, unsigned char* bufspace, unsigned bufsize)
 *                                          src/lib/cimbar_js/cimbar_recv_js.h:17; get_rgb, cimbar_recv_js.cpp:94-120; `format <= 0` is 3, :150-151
 * whose only camera caller hands over VideoFrames as they come: NV12 (12), I420 (420) or RGBA (4) (web/recv-worker.js:38-47, web/recv.js:110,362-371).
 * The four entry points above with that argument in the reference's position (after the height). `img` = n captures of
 * cimbar_hip_capture_bytes(width, height, format) bytes each, back to back:
 *   3 (and <= 0, and any value the reference's `default:` lets through)  RGB8, width * height * 3
 *   4    RGBA8, width * height * 4; the alpha byte is dropped (cv::COLOR_RGBA2RGB)
 *   12   NV12: width * height luma bytes, then height / 2 rows of width bytes (U, V, U, V ...)        (cv::COLOR_YUV2RGB_NV12)
 *   420  three planes: width * height luma, then two (width / 2) x (height / 2) chroma planes, read the way the reference's conversion code
 *        cv::COLOR_YUV420p2RGB reads them -- OpenCV defines it as COLOR_YUV2RGB_YV12: the FIRST chroma plane is V. (An I420 VideoFrame has U
 *        first; upstream decodes such captures with red and blue exchanged and leaves it to the header-derived colour correction. Kept.)
 * YUV -> RGB is OpenCV's fixed-point BT.601, gray / blur / warp then see exactly the RGB image get_rgb would have built -- but no
 * such image is ever written: the scan and warp kernels convert as they load, so a 1080p NV12 capture costs 3.1 MB of PCIe and HBM reads
 * instead of 6.2. 12 and 420 need an even width and height (cv::cvtColor asserts it; upstream throws): CIMBAR_HIP_EDIM, and
 * cimbar_hip_capture_bytes returns 0. Everything else as for the entry point without the suffix (which is format 3).
 * cimbard_scan_extract_decode(img, w, h, format, buf, size) is then
 *   cimbar_hip_scan_extract_decode_batch_fmt(ctx, img, w, h, format, 1, CIMBAR_HIP_MEM_HOST, 1, 2, chunks, &mask, &status, CIMBAR_HIP_MEM_HOST, NULL)
 * (upstream always sharpens on this path: `bool shouldPreprocess = true`, cimbar_recv_js.cpp:166) with status 0 -> return -3 and the chunks
 * whose mask bit is set packed front to back (escrow_buffer_writer); INTEGRATION.md has the wrapper.
 *
 * Capture formats of native receivers. Those four are what a browser hands over; cv::VideoCapture, V4L2 and the Android camera deliver others,
 * which the reference's native front ends convert on the host first (cv::cvtColor(COLOR_BGR2RGB), recv.cpp:139). Five more values of `format`,
 * each defined by the cvtColor code that builds the same RGB image, converted as loaded like the four above:
 *   21    NV21: NV12 with every chroma pair stored (V, U); width * height * 3 / 2, even width and height             (cv::COLOR_YUV2RGB_NV21)
 *   422   YUYV / YUY2: width * height * 2; a row is width / 2 groups (Y0, U, Y1, V); the (U, V) pair serves the two pixels of its group
 *         and no other row; even width, any height                                                                   (cv::COLOR_YUV2RGB_YUY2)
 *   4221  UYVY: the same with the group stored (U, Y0, V, Y1)                                                        (cv::COLOR_YUV2RGB_UYVY)
 *   30    BGR8: width * height * 3, stored B, G, R                                                                   (cv::COLOR_BGR2RGB)
 *   40    BGRA8: width * height * 4, stored B, G, R, A; the alpha byte is dropped                                    (cv::COLOR_BGRA2RGB)
 * The YUV ones use the same fixed-point BT.601 arithmetic as 12 / 420 (OpenCV runs 4:2:2 through the code of 4:2:0). A width or height the layout
 * cannot hold: CIMBAR_HIP_EDIM, cimbar_hip_capture_bytes 0. Every value that is none of the nine stays RGB8. Every entry point that takes `format`
 * takes them (the _fmt calls here, the combined / stitched / stream _fmt calls, cimbar_hip_auto_scan_extract_decode_batch_fmt, the undistort
 * calls); libcimbar_recv_hip.so, being the reference's interface, keeps the reference's meaning (anything but 4 / 12 / 420 is RGB8).
 * Not covered: row pitch / plane strides of padded camera and video-decoder surfaces (captures are densely packed), Bayer raw, 10-bit formats,
 * the ingest library, cimbar_hip_decode_frame (RGB8 with a stride). */
enum cimbar_hip_format {
	CIMBAR_HIP_FMT_RGB = 3,
	CIMBAR_HIP_FMT_RGBA = 4,
	CIMBAR_HIP_FMT_NV12 = 12,
	CIMBAR_HIP_FMT_I420 = 420,       /* as cv::COLOR_YUV420p2RGB reads it: see above */
	CIMBAR_HIP_FMT_NV21 = 21,
	CIMBAR_HIP_FMT_YUYV = 422,
	CIMBAR_HIP_FMT_UYVY = 4221,
	CIMBAR_HIP_FMT_BGR = 30,
	CIMBAR_HIP_FMT_BGRA = 40
};
size_t cimbar_hip_capture_bytes(unsigned width, unsigned height, int format);
int cimbar_hip_scan_preprocess_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n, int img_mem,
                                   uint8_t* binary, int* thresholds, int out_mem, void* hip_stream);
int cimbar_hip_deskew_batch_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n, int img_mem,
                                const float* corners, uint8_t* frames, int out_mem, void* hip_stream);
int cimbar_hip_extract_batch_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n, int img_mem,
                                 uint8_t* frames, int* status, float* corners, int out_mem, void* hip_stream);
int64_t cimbar_hip_scan_extract_decode_batch_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n,
                                                 int img_mem, int preprocess, int color_correction, uint8_t* chunks, uint32_t* masks, int* status,
                                                 int out_mem, void* hip_stream);

/* ---- mode auto-detection: captures whose mode is not known ----------------------------------------------------------------------------
 * The reference's web receiver in its default auto mode (web/recv.js:112,346,378) tries the modes [66, 68, 67, 4] in turn, each try being
 * cimbard_configure_decode(mode) + cimbard_scan_extract_decode, and locks onto the first mode that returns bytes. An auto-detection object holds
 * one decoder per candidate mode and ONE carried colour-correction matrix, shared by every mode -- as the reference's thread_local one is
 * (CimbDecoder.cpp:69-73; cimbard_configure_decode leaves it alone, cimbar_recv_js.cpp:272-288).
 *
 * cimbar_hip_auto_create: `modes` = n_modes distinct values of 68 67 66 4 8 (anything else, a repeat or n_modes outside 1..5: CIMBAR_HIP_EINVAL).
 *   The carried matrix starts inactive. cimbar_hip_auto_bufsize = the per-capture slot stride = the largest cimbar_hip_mode_bufsize of the modes.
 * cimbar_hip_auto_scan_extract_decode_batch_fmt: for each capture IN BATCH ORDER the result is that of this loop on one thread of the reference:
 *       for m in candidates: Config::update(m); r = extract + Decoder::decode_fountain in mode m (preprocess, color_correction as given);
 *                            if r > 0: accept m, stop
 *   with the matrix carried across captures, candidates and calls. Candidates: `order` (n_order distinct modes the object was created with, tried
 *   in that order; a caller that has locked onto a mode passes just that one), or NULL = the creation order. Per capture f:
 *     modes_out[f] = the accepted mode, 0 if no candidate delivered a chunk (or the extractor found no frame);
 *     chunks[f * cimbar_hip_auto_bufsize + j * chunk_size(modes_out[f]) ..] = slot j of the accepted attempt, masks[f] its delivered slots, the
 *       rest of the capture's slot zero (a capture with mode 0: all zero, mask 0);
 *     status[f] = the extraction status (0 FAILURE, 1 SUCCESS, 2 NEEDS_SHARPEN) of the accepted attempt, or of the first candidate where none was
 *       accepted (it only differs between modes in NEEDS_SHARPEN, which depends on the target size: Corners::is_granular_scale).
 *   `format`, `preprocess` (1 / 0 / -1), img_mem / out_mem and hip_stream as for cimbar_hip_scan_extract_decode_batch_fmt. Returns the good bytes
 *   over the batch, for device outputs too: the call reads back one count per candidate and one flag per settling round (the acceptance is
 *   guessed from the symbol halves and checked after the colour halves; DESIGN_WIDENING.md "Mode detection"), so it always returns complete.
 *   Erasure decoding, multi-capture combining and undistortion are not offered here. CIMBAR_HIP_EINVAL / _EDIM / _EHIP as the neighbouring
 *   entry points, the message in cimbar_hip_auto_last_error.
 * cimbar_hip_auto_reset_ccm / _get_ccm / _set_ccm: the ONE carried matrix, as cimbar_hip_reset_ccm / _get_ccm / _set_ccm for a context. */
typedef struct cimbar_hip_auto cimbar_hip_auto;
int cimbar_hip_auto_create(int device, const int* modes, int n_modes, cimbar_hip_auto** out);
void cimbar_hip_auto_destroy(cimbar_hip_auto* a);
int cimbar_hip_auto_bufsize(const cimbar_hip_auto* a);
const char* cimbar_hip_auto_last_error(const cimbar_hip_auto* a);
int cimbar_hip_auto_reset_ccm(cimbar_hip_auto* a);
int cimbar_hip_auto_get_ccm(cimbar_hip_auto* a, float out9[9]);
int cimbar_hip_auto_set_ccm(cimbar_hip_auto* a, const float m9[9]);
int64_t cimbar_hip_auto_scan_extract_decode_batch_fmt(cimbar_hip_auto* a, const int* order, int n_order, const uint8_t* img, unsigned width,
                                                      unsigned height, int format, int n, int img_mem, int preprocess, int color_correction,
                                                      uint8_t* chunks, uint32_t* masks, int* modes_out, int* status, int out_mem, void* hip_stream);

/* ---- lens undistortion: `cimbar --undistort` (src/exe/cimbar/cimbar.cpp:135-145) -----------------------------------------------------------
 * Undistort<SimpleCameraCalibration> (src/lib/extractor/Undistort.h:11-62) in front of Extractor::extract, on the device. Captures as for the _fmt
 * entry points above (`format`, img_mem, out_mem, hip_stream, ctx->err via cimbar_hip_last_error on failure).
 *
 * cimbar_hip_undistort_calibrate_fmt: SimpleCameraCalibration::scan (SimpleCameraCalibration.h:30-58, .cpp:1-75) per capture -- Scanner's anchor
 *   search, Scanner::scan_edges (Scanner.cpp:204-276) and calculate_distortion_factor. ok[f] = 1 with k1[f] = the distortion factor where the
 *   reference returns parameters (no edge found at all still counts: k1 = 0), ok[f] = 0 and k1[f] = 0 where it returns {} (fewer than 4 anchors;
 *   opposite sides parallel, which an axis-aligned capture without perspective has). The camera is naive_radial_undistort's
 *   [w/4, 0, w/2; 0, h/4, h/2; 0, 0, 1] (integer division), the distortion (k1, 0, 0, 0). ok and k1 are host arrays of n; complete on return.
 *   Where Scanner::chase_edge would read outside the image (undefined behaviour upstream), the pixel counts as inactive.
 *
 * cimbar_hip_undistort_batch_fmt: Undistort::undistort(img, out) with a fresh object per capture (what cimbar.cpp:139 does), i.e.
 *   cv::initUndistortRectifyMap(camera, dist, Mat(), camera, size, CV_32FC1) + cv::remap(INTER_LINEAR, BORDER_CONSTANT 0):
 *   out_rgb = n undistorted RGB8 captures of width x height (any width), whatever the input format.
 *   params == NULL: calibrate each capture as above; a capture whose calibration fails gets ok = 0 and its plain RGB conversion (the CLI's img
 *                   stays as it was).
 *   params != NULL: 14 doubles, camera[9] (row-major) + distortion[5] (k1 k2 p1 p2 k3), applied to all n captures (set_distortion_params): ok = 1,
 *                   k1_out = params[9]. Only zero-skew cameras [fx, 0, cx; 0, fy, cy; 0, 0, 1] (finite, non-singular): anything else is
 *                   CIMBAR_HIP_EINVAL.
 *   ok / k1_out (n each, may be NULL) follow out_mem. Host outputs: complete on return; device outputs: enqueued.
 *
 * cimbar_hip_scan_undistort_extract_decode_batch_fmt: cimbar_hip_scan_extract_decode_batch_fmt with `--undistort` -- the body of cimbar.cpp:124-162:
 *   calibrate, remap, extract, decode, nothing crossing PCIe in between. undistort_ok (n, may be NULL; follows out_mem) = the calibration's ok.
 *   Everything else as for cimbar_hip_scan_extract_decode_batch_fmt.
 *
 * Bounds: the undistorted captures live in a context-owned scratch allocated on the first call of these entry points (none of the others touch
 * it) and holding at most 256 MiB (CIMBAR_HIP_UNDISTORT_SCRATCH_MB): a batch goes through in groups of that many captures (43 at 1920x1080), at least
 * one. Staged host input, the scan state and the deskewed frames of the composite are as large as for the entry points above. */
int cimbar_hip_undistort_calibrate_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n, int img_mem,
                                       int* ok, double* k1, void* hip_stream);
int cimbar_hip_undistort_batch_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n, int img_mem,
                                   const double* params, uint8_t* out_rgb, int out_mem, int* ok, double* k1_out, void* hip_stream);
int64_t cimbar_hip_scan_undistort_extract_decode_batch_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n,
                                                           int img_mem, int preprocess, int color_correction, uint8_t* chunks, uint32_t* masks,
                                                           int* status, int* undistort_ok, int out_mem, void* hip_stream);

/* ---- multi-GPU: the one exchange step ------------------------------------------------------------------------------------
 * Frames are independent, so each GPU decodes its own slab with its own context; afterwards every rank's n x (7500 chunk bytes + 1 mask
 * word) are gathered on `root` in rank order (== frame order for contiguous slabs), where the host feeds the single fountain_decoder_sink
 * -- the shape of the reference's worker pool -> one sink (web/recv-worker.js:47-64, web/recv.js:36). The gather is ncclGather over RCCL /
 * xGMI (/opt/rocm/include/rccl/rccl.h:745); RCCL is loaded on first use, the library does not link against it.
 *   comm_init_all   : one process driving ndev GPUs (one context + one comm per device; call gather_chunks from one thread per device or
 *                     inside the caller's own group). devices NULL = 0..ndev-1. Fills out[0..ndev).
 *   comm_unique_id / comm_init_rank : one process per GPU; rank 0 makes the 128-byte id and hands it to the others by its own means.
 *   gather_chunks   : chunks / masks: this rank's n frames (device memory); all_chunks / all_masks: nranks * n frames on root (device
 *                     memory, may be NULL elsewhere). Enqueued on hip_stream; returns 0.
 *   comm_info       : the communicator's size and this member's rank as RCCL reports them (ncclCommCount / ncclCommUserRank): what a
 *                     benchmark line quotes so that it says itself how many ranks the exchange ran over. */
typedef struct cimbar_hip_comm cimbar_hip_comm;
int cimbar_hip_comm_init_all(int ndev, const int* devices, cimbar_hip_comm** out);
int cimbar_hip_comm_unique_id(uint8_t id128[128]);
int cimbar_hip_comm_init_rank(const uint8_t id128[128], int nranks, int rank, int device, cimbar_hip_comm** out);
int cimbar_hip_comm_info(cimbar_hip_comm* comm, int* nranks, int* rank);
void cimbar_hip_comm_destroy(cimbar_hip_comm* comm);
int cimbar_hip_gather_chunks(cimbar_hip_ctx* ctx, cimbar_hip_comm* comm, int root, const uint8_t* chunks, const uint32_t* masks, int n,
                             uint8_t* all_chunks, uint32_t* all_masks, void* hip_stream);
/* The same exchange for the batch issued LAST through cimbar_hip_decode_batch_pipelined, enqueued on that batch's own pipeline stream right behind its
 * kernels (chunks / masks = the buffers that call was given): no stream or event of the caller's is involved, and cimbar_hip_pipeline_wait -- which a
 * consumer of the batch calls anyway -- then also covers all_chunks / all_masks on the root. Every rank calls it after every pipelined batch, in the same
 * order. This is what bench.py's N > 1 loop issues per step. CIMBAR_HIP_EINVAL if no pipelined batch has been issued on the context. */
int cimbar_hip_pipeline_gather(cimbar_hip_ctx* ctx, cimbar_hip_comm* comm, int root, const uint8_t* chunks, const uint32_t* masks, int n,
                               uint8_t* all_chunks, uint32_t* all_masks);

/* ---- PNG decode on the device (what cv::imread does in front of the decoder, cimbar.cpp:132-133) --------------------
 * A batch of PNG images whose zlib streams (the concatenated IDAT payloads) already sit in device memory -> dense RGB8 frames in device
 * memory, without the decoded pixels ever crossing PCIe: inflate (one wavefront per image, Huffman decode + LZ77 window in LDS, Adler-32
 * checked) and the scanline un-filter (rows skewed over the lanes). 8 bits per sample, non-interlaced, colour types 0 (gray, replicated),
 * 2 (RGB), 3 (palette), 6 (RGBA, alpha dropped) -- what cv::imread(IMREAD_COLOR) + BGR2RGB gives; at most 2048 pixels wide (frames are
 * 1024 or 736). Context-free: `device` is a HIP ordinal.
 *   d_zbuf / zbuf_bytes : the streams (and palettes), device memory. The kernels read whole dwords: every stream's end rounded up to a multiple
 *                         of 4 must lie inside zbuf_bytes (checked; an image whose padded end does not is refused with EHEADER)
 *   d_desc              : n descriptors, device memory
 *   d_scratch           : n * scratch_stride bytes for the filtered scanlines; scratch_stride >= cimbar_hip_png_scratch_bytes(), multiple of 16
 *   d_rgb               : n * rgb_stride bytes; image i's width*height*3 bytes start at i * rgb_stride
 *   d_status            : n words: 0 or a CIMBAR_HIP_PNG_E* code per image (a refused image leaves its rgb slot undefined)
 * Enqueued on hip_stream; returns 0, or a negative code if the launch itself failed. libcimbar_ingest.so's device mode
 * (include/cimbar_ingest.h) is the host side that parses the files and fills these buffers. */
enum {
	CIMBAR_HIP_PNG_EHEADER = -30,   /* descriptor / zlib header not acceptable (colour type, size, window, preset dictionary, alignment) */
	CIMBAR_HIP_PNG_ESTREAM = -31,   /* invalid deflate stream (block type, stored length, distance too far back, invalid code, truncated, filter type) */
	CIMBAR_HIP_PNG_ECODES = -32,    /* over-subscribed or incomplete Huffman code set (zlib's inflate_table rules) */
	CIMBAR_HIP_PNG_ESIZE = -33,     /* the stream inflates to more or fewer bytes than height * (1 + width * bytes per pixel), or the slot is too small */
	CIMBAR_HIP_PNG_ECHECK = -34     /* Adler-32 mismatch */
};
typedef struct cimbar_hip_png_desc {
	uint64_t zoff;        /* byte offset of the image's zlib stream in d_zbuf, a multiple of 16 */
	uint32_t zlen;        /* its length, below 256 MiB (bit positions are 32-bit) */
	uint32_t width, height;
	uint32_t color_type;  /* 0, 2, 3, 6 */
	uint32_t pal_off;     /* colour type 3: byte offset in d_zbuf of 256 RGB palette entries (768 bytes) */
	uint32_t reserved;
} cimbar_hip_png_desc;
size_t cimbar_hip_png_scratch_bytes(unsigned width, unsigned height, unsigned color_type);
int cimbar_hip_png_decode_batch(int device, const uint8_t* d_zbuf, size_t zbuf_bytes, const cimbar_hip_png_desc* d_desc, int n, uint8_t* d_scratch,
                                size_t scratch_stride, uint8_t* d_rgb, size_t rgb_stride, int32_t* d_status, void* hip_stream);
/* the same with a hint about the launch: 0 = decide by n (what the call above does), 1 = one stream per wavefront (shortest time for a lone
 * launch of up to a few thousand images), 4 = "8192+ images are in flight", whether in one launch or in several concurrent ones (what the
 * ingest library's device mode keeps going). For 4 (and for 0 with n >= 8192) the DEVICE picks the inflate kernel: streams of long matches
 * (frames as Pillow writes them) are fastest four to a wavefront, streams with short literal codes (cv::imwrite's defaults: the reference
 * encoder's files) through the one-stream kernel's all-offsets turn; the first image's first block decides for the launch. */
int cimbar_hip_png_decode_batch_v(int device, const uint8_t* d_zbuf, size_t zbuf_bytes, const cimbar_hip_png_desc* d_desc, int n, uint8_t* d_scratch,
                                  size_t scratch_stride, uint8_t* d_rgb, size_t rgb_stride, int32_t* d_status, int variant, void* hip_stream);

/* ---- stage taps (parity tests / profiling; all buffers host memory, sized for the LAST decoded batch of n frames) --- */
enum {
	CIMBAR_HIP_TAP_BITPLANE = 0,   /* n * 131072 bytes: CimbReader::_grayscale layout (bit x+1024*y, MSB first) */
	CIMBAR_HIP_TAP_SYMBOLS = 1,    /* n * 12400 bytes : symbol (0..15) by linear cell index */
	CIMBAR_HIP_TAP_COLORS = 2,     /* n * 12400 bytes : colour (0..3) by linear cell index */
	CIMBAR_HIP_TAP_DRIFT = 3,      /* n * 12400 * 2 int8: accumulated (dx,dy) at which each cell's colour is read */
	CIMBAR_HIP_TAP_RS_OK = 4,      /* n * 60 bytes    : 1 = libcorrect-equivalent decode returned > 0, per RS block */
	CIMBAR_HIP_TAP_FLOOD = 5,      /* n bytes         : 1 = frame left the parallel pass: a flood pass decoded it (CIMBAR_HIP_TAP_FLOOD_PATH says which:
	                                  the exact flood-order replay, the certified batch flood or, with cimbar_hip_set_relaxed_flood, the rounds) */
	CIMBAR_HIP_TAP_CCM = 6,        /* n * 10 floats   : 3x3 matrix used for the colour pass + active flag */
	CIMBAR_HIP_TAP_FLOOD_PATH = 7, /* n bytes         : 0 = parallel pass was exact, 1 = exact flood replay, 2 = certified batch flood,
	                                  3 = flooded in rounds, accepted (cimbar_hip_set_relaxed_flood; without its fallback: flooded in rounds) */
	CIMBAR_HIP_TAP_FLOOD_INFO = 8, /* n u32           : what the batch-parallel flood made of a flagged frame: low byte 0 = certified, 1..4 = the rule
	                                  that declined it, 5 = out of super-rounds; bits 8..15 the super-round; bits 16.. cells decoded by then.
	                                  0xFFFFFFFF for frames that were never flagged, and for every frame of a batch in which the pass did not
	                                  run: after a batch where it certified fewer than one in sixteen of the frames it was given, the next fifteen
	                                  batches go straight to the exact replay (CIMBAR_HIP_FLOOD_WAVE_ADAPT=0 at cimbar_hip_create: never skip).
	                                  Which pass produced a frame's symbols never changes them */
	CIMBAR_HIP_TAP_FLOOD_VERIFY = 9, /* n u32         : with CIMBAR_HIP_FLOOD_VERIFY=1 in the environment at cimbar_hip_create, every frame the batch-parallel
	                                  flood certified is ALSO replayed exactly and compared: cells whose symbol or drifted position differed
	                                  (0 = the certificate held; the exact result is what the decode used either way); 0xFFFFFFFF for frames
	                                  that were not certified, or when the mode is off. The context prints the totals to stderr at destroy. */
	/* the group decode of the last batch, when it was a combined one (cimbar_hip_decode_batch_combined / _scan_extract_decode_batch_combined_fmt;
	 * CIMBAR_HIP_EINVAL after any other batch). The taps above keep describing that batch's per-capture decode. */
	CIMBAR_HIP_TAP_GROUP_CELLS = 10,  /* n_groups * cells bytes: the group's combined cell, colour << 4 | symbol */
	CIMBAR_HIP_TAP_GROUP_MARGIN = 11, /* n_groups * cells u16  : the symbol's margin, 0xFFFF where the members' symbols agree */
	CIMBAR_HIP_TAP_GROUPS = 12,       /* n int32               : the group of every capture, -1 for none */
	/* the colour retry of the last batch (cimbar_hip_set_colour_erasure_decode; CIMBAR_HIP_EINVAL when that batch ran with the setting off) */
	CIMBAR_HIP_TAP_COLOUR_MARGIN = 13,/* n * cells u32         : the classifier's margin of every cell, by linear cell index, of the frames the retry
	                                     worked on; 0xFFFFFFFF for all cells of a frame it skipped (all colour chunks in the mask) */
	/* the anchor search of the last extract / scan_extract_decode call (n = that call's captures; valid without any decoded batch; an entry point that
	 * searches its captures in several pieces describes the last piece) */
	CIMBAR_HIP_TAP_SCAN_PATH = 14,    /* n int32               : 0 = the fast search kernels answered, 1 = one of their fixed lists overflowed and the
	                                     serial search answered, 2 = gave up (more than 16 overflowing captures in the batch, or the serial search's
	                                     own lists overflowed): the capture is reported as a failure */
	/* the colour vote of the last combined batch: a plain one with cimbar_hip_set_group_colour_vote on, or a stream call of a stream with
	 * cimbar_hip_set_stream_colour_vote on (CIMBAR_HIP_EINVAL when that batch ran with its setting off or was no combined batch). After a stream
	 * call n_groups counts the groups closed in it and n its own captures. */
	CIMBAR_HIP_TAP_GROUP_COLOUR_MARGIN = 15, /* n_groups * cells u32: the group colour margin gm, 0xFFFFFFFF where the members' colours all agree */
	CIMBAR_HIP_TAP_GROUP_COLOUR_WEIGHTS = 16,/* n * cells u32       : the weight each capture contributed to its group's vote; 0 for cells without a
	                                            colour dispute and for captures in no group (stream call: in no group that closed in the call) */
	/* the carry store after the last batch, when that was a stream call of a stream with cimbar_hip_set_stream_colour_vote on (else
	 * CIMBAR_HIP_EINVAL) */
	CIMBAR_HIP_TAP_STREAM_CARRY_WEIGHTS = 17,/* rows * cells u32    : the carried weights of slots 0 .. rows - 1 (the open group's members in capture
	                                            order), every cell filled; rows = out_bytes / (cells * 4), CIMBAR_HIP_EINVAL above the occupied slots */
	/* the stitching of the last batch, when it was a stitched one (cimbar_hip_decode_batch_stitched / _scan_extract_decode_batch_stitched_fmt;
	 * CIMBAR_HIP_EINVAL after any other batch). After a stitched-stream call of n captures both describe its n rows: 2n * cells bytes and
	 * n * L u16, row 0 first (zero counts where row 0 had no usable carry). */
	CIMBAR_HIP_TAP_STITCH_CELLS = 18, /* 2 (n - 1) * cells bytes: the stitched cell of slot 2k + d, colour << 4 | symbol; zero for the slots of a
	                                     pair that is no candidate */
	CIMBAR_HIP_TAP_STITCH_LINES = 19, /* (n - 1) * L u16        : cnt(l), the agreeing cells of pair k on line l of the call's axis */
	/* what the stitched-stream calls carry: the last capture of the last such call (CIMBAR_HIP_EINVAL while nothing is carried: after create and
	 * after cimbar_hip_stitch_stream_reset); does not depend on the last batch */
	CIMBAR_HIP_TAP_STITCH_CARRY = 20, /* 2 * cells bytes        : the carried symbols, then the carried colours, by linear cell index */
	/* the threshold kernel's second product, as it left it (the colour pass reads it where a cell has no drift) */
	CIMBAR_HIP_TAP_CELL_MEANS = 21,   /* n * grid slots u32     : r | g << 8 | b << 16, the inner-6x6 mean (Cell.h: channel sum / 36, remainder dropped) of
	                                     every cell at its undrifted position, by grid slot row * columns + column (112 x 112 | 112 x 78 | 80 x 69
	                                     slots, the four corner cut-outs included) */
	/* the strips of the last batch, when it was a stitched one that ran with cimbar_hip_set_stitch_strips = S above 1 (else CIMBAR_HIP_EINVAL);
	 * rows = n - 1, after a stitched-stream call n. CIMBAR_HIP_TAP_STITCH_LINES of such a batch is cnt(l) = the sum of cnt(l, j) over j. */
	CIMBAR_HIP_TAP_STITCH_STRIPS = 22,      /* rows * S * 4 int32: {a_j, b_j, s_j, f_j}; a_j = b_j = -1 for a strip that is not located, s_j = the
	                                           resolved split, -1 in a pair that is no candidate */
	CIMBAR_HIP_TAP_STITCH_STRIP_LINES = 23, /* rows * S * L u16  : cnt(l, j), the agreeing cells of line l in strip j */
	/* what the stage in front of the anchor search left for the captures CIMBAR_HIP_TAP_SCAN_PATH describes (n = the captures of the last
	 * search launch, w x h their size; CIMBAR_HIP_EINVAL before any search). Read them before the next call of the extractor stage:
	 * cimbar_hip_scan_preprocess runs no search, but writes its own histograms and thresholds where these two taps read */
	CIMBAR_HIP_TAP_SCAN_GRAY = 24,      /* n * w * h bytes     : the blurred gray plane the search read, row-major, capture after capture */
	CIMBAR_HIP_TAP_SCAN_HIST = 25,      /* n * 256 u32         : the histogram of each plane */
	CIMBAR_HIP_TAP_SCAN_THRESHOLD = 26, /* n int32             : the Otsu threshold of each histogram; the search reads gray > threshold */
	/* the relaxed flood of the last batch (cimbar_hip_set_relaxed_flood) */
	CIMBAR_HIP_TAP_FLOOD_ROUNDS = 27,   /* n u32              : rounds | cells decoded << 16 of every frame flooded in rounds -- also of one that was
	                                       then handed to the exact replay (CIMBAR_HIP_TAP_FLOOD_PATH 1); 0 for every other frame, and for every
	                                       frame of a batch that ran with the setting off */
	/* the grouping of the last once-call (cimbar_hip_decode_batch_once / _scan_extract_decode_batch_once_fmt; n = its captures;
	 * CIMBAR_HIP_EINVAL before any). After a once-stream call (cimbar_hip_decode_batch_once_stream / _scan_extract_decode_batch_once_stream_fmt)
	 * they describe its n captures, and _AGREE has n entries: entry 0 is capture 0 against the carried capture (0 when the carry is
	 * unusable or nothing is carried), entry k is agree(k - 1, k). */
	CIMBAR_HIP_TAP_REPEAT_SIG = 28,     /* n * cells bytes     : sig_c, 0..3, by linear cell index */
	CIMBAR_HIP_TAP_REPEAT_AGREE = 29,   /* (n - 1) u32         : agree(k, k + 1); after a once-stream call n u32 */
	/* what the once-stream calls carry: the last capture of the last such call (CIMBAR_HIP_EINVAL while nothing is carried: after create and
	 * after cimbar_hip_once_stream_reset); does not depend on the last batch */
	CIMBAR_HIP_TAP_REPEAT_CARRY = 30,   /* cells bytes + 3 u32 : the carried signature, then {usable, len, P}; len and P are 0 when usable is */
	/* the run rescue of the last once-call (cimbar_hip_set_once_rescue; n = its captures). CIMBAR_HIP_EINVAL when that call ran with the
	 * setting off or was a once-stream call. A call with the setting on that tried nothing (rchunks and rmasks both NULL included) reports
	 * n times -1 and no cells. _CELLS reads the group scratch the combined calls share: ask before the next combined call on the context. */
	CIMBAR_HIP_TAP_ONCE_RESCUE = 31,    /* n int32             : per run slot, -1 = the run was not tried, else the chunk bits the rescue added to the OR
	                                       of the members' masks; slots at and above the run count are -1 */
	CIMBAR_HIP_TAP_ONCE_RESCUE_CELLS = 32, /* tried * cells bytes : the combined cells of the tried runs, in run order, colour << 4 | symbol */
	/* tear skipping in the last once-call (cimbar_hip_set_once_tear_skip; n = its captures). CIMBAR_HIP_EINVAL when that call ran with the
	 * setting off or was a once-stream call */
	CIMBAR_HIP_TAP_ONCE_TEAR = 33,      /* n x 4 int32         : per capture {axis * 2 + o, s, first, last}; {-1, -1, 0, 0} for a capture that is no candidate */
	/* which launches of the exact flood replay (k_flood3) the last batch of any kind made on the host side: bookkeeping only, answered without
	 * waiting for the device, so it may be asked while pipelined batches are in flight. It describes the batch issued last (each batch starts
	 * its own list). Record 0 is a header {areas asked for, areas held, launches, 0, 0, 0, 0}: the spill areas that batch needed [0, asked)
	 * and the areas the context holds now (>= asked; it only grows). One record per launch follows, in issue order, at most 16 (later ones are
	 * dropped): instance = 3, 4 or 8 frames per CU (heap slots in LDS: 10 240, 7 080, 4 095); a launch with grid < frames hands the frames from
	 * `grid` on out through counter pair `counter`; workgroup b spills into area area0 + b; flags says which frames the launch was for. */
	CIMBAR_HIP_TAP_FLOOD_LAUNCH = 34,   /* (1 + launches) x 7 int32: {instance, grid, frames, first frame, area0, counter, flags: 0 = the batch's flags,
	                                       1 = the verify replay (CIMBAR_HIP_FLOOD_VERIFY), 2 = the relaxed flood's fallback replay}; returns the bytes written */
	/* tear salvage in the last once-call (cimbar_hip_set_once_tear_salvage; n = its captures). CIMBAR_HIP_EINVAL when the setting was not
	 * effective in that call, or it was a once-stream call */
	CIMBAR_HIP_TAP_ONCE_SALVAGE = 35,   /* n x 8 int32         : per run slot {kp, axis_p, lo_p, hi_p, kf, axis_f, lo_f, hi_f}, the preceding and the following
	                                       partial of the run with their line ranges; {-1, -1, 0, 0} for a partial the run does not have, and for
	                                       both partials of a run that was not tried */
	/* the erasure retry of the last batch's stitched decode (cimbar_hip_set_stitch_erasure). CIMBAR_HIP_EINVAL when that batch was not a plain
	 * stitched call that ran the respective retry (the setting off, its erasure setting off, a stitched-stream call, n == 1) */
	CIMBAR_HIP_TAP_STITCH_DISTANCE = 36,      /* 2 (n - 1) * cells u8 : d_sym of every cell of slot 2k + d, by linear cell index; 0xFF for every
	                                             cell of a slot the symbol retry skipped (not live, or no symbol chunk missing) */
	CIMBAR_HIP_TAP_STITCH_COLOUR_MARGIN = 37  /* 2 (n - 1) * cells u32: margin of every cell of the slot; 0xFFFFFFFF for a slot the colour retry
	                                             skipped */
};
int64_t cimbar_hip_tap(cimbar_hip_ctx* ctx, int what, void* out, size_t out_bytes);

/* Average device time (ms) of each pipeline stage over the last decode_batch call that ran with timing enabled
 * (HIP events on the launch stream). names: static strings. Returns the number of stages written (<= max). */
int cimbar_hip_enable_timing(cimbar_hip_ctx* ctx, int on);
int cimbar_hip_stage_times(cimbar_hip_ctx* ctx, const char** names, float* ms, int max);

#ifdef __cplusplus
}
#endif
#endif /* CIMBAR_HIP_H */
