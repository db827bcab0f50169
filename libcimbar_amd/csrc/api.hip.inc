// api.hip.inc -- part of cimbar_hip.hip: the extern "C" entry points of include/cimbar_hip.h. The geometry-dependent implementation exists once
// per mode (mode.hip.inc -> namespaces m68, m67, m66, m4, m8); a context remembers its mode in its first word and every call is forwarded to that copy.
namespace {

inline int ctx_mode(const cimbar_hip_ctx* ctx) { return *reinterpret_cast<const int*>(ctx); }

#define CIMBAR_FWD(fn, ...)                                                                          \
	(ctx_mode(ctx) == 67 ? m67::fn((m67::cimbar_hip_ctx*)ctx, ##__VA_ARGS__)                         \
	 : ctx_mode(ctx) == 66 ? m66::fn((m66::cimbar_hip_ctx*)ctx, ##__VA_ARGS__)                       \
	 : ctx_mode(ctx) == 4 ? m4::fn((m4::cimbar_hip_ctx*)ctx, ##__VA_ARGS__)                          \
	 : ctx_mode(ctx) == 8 ? m8::fn((m8::cimbar_hip_ctx*)ctx, ##__VA_ARGS__)                          \
	                       : m68::fn((m68::cimbar_hip_ctx*)ctx, ##__VA_ARGS__))

// what comm.hip.inc needs of a context
inline void ctx_view(cimbar_hip_ctx* ctx, int* device, std::string** err, int* frame_bytes) { CIMBAR_FWD(ctx_view, device, err, frame_bytes); }

inline bool ctx_pipe_view(cimbar_hip_ctx* ctx, hipStream_t* stream, hipEvent_t* done) { return CIMBAR_FWD(ctx_pipe_view, stream, done); }

inline deliver::View delivery_view(cimbar_hip_ctx* ctx)
{
	deliver::View v;
	CIMBAR_FWD(delivery_view, &v);
	return v;
}

}  // namespace

extern "C" {

int cimbar_hip_create(int device, int mode_val, cimbar_hip_ctx** out)
{
	if (!out) return CIMBAR_HIP_EINVAL;
	*out = nullptr;
	switch (mode_val) {
		case 68: return m68::cimbar_hip_create(device, 68, (m68::cimbar_hip_ctx**)out);
		case 67: return m67::cimbar_hip_create(device, 67, (m67::cimbar_hip_ctx**)out);
		case 66: return m66::cimbar_hip_create(device, 66, (m66::cimbar_hip_ctx**)out);
		case 4: return m4::cimbar_hip_create(device, 4, (m4::cimbar_hip_ctx**)out);
		case 8: return m8::cimbar_hip_create(device, 8, (m8::cimbar_hip_ctx**)out);
		default: return m68::cimbar_hip_create(device, 68, (m68::cimbar_hip_ctx**)out);   // Config::temp_conf's `case 68: default:` (Config.h:41-43): any other value is mode B
	}
}

void cimbar_hip_destroy(cimbar_hip_ctx* ctx)
{
	if (!ctx) return;
	CIMBAR_FWD(cimbar_hip_destroy);
}

int cimbar_hip_bufsize(void) { return m68::cimbar_hip_bufsize(); }   // the default configuration's frame payload (a thread that never called Config::update)

int cimbar_hip_mode_bufsize(int mode_val)                             // ... of the configuration Config::update(mode_val) selects (Config.h:19-44: anything unlisted is mode B)
{
	switch (mode_val) {
		case 67: return m67::cimbar_hip_bufsize();
		case 66: return m66::cimbar_hip_bufsize();
		case 4: return m4::cimbar_hip_bufsize();
		case 8: return m8::cimbar_hip_bufsize();
		default: return m68::cimbar_hip_bufsize();
	}
}

int cimbar_hip_ctx_bufsize(const cimbar_hip_ctx* ctx)                 // cimbard_get_bufsize() of the context's configuration (cimbar_recv_js.cpp:143-146)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_ctx_bufsize);
}

int cimbar_hip_tile_hashes(uint64_t out16[16]) { return m68::cimbar_hip_tile_hashes(out16); }   // the tile set is the same for every 8x8 mode

const char* cimbar_hip_last_error(const cimbar_hip_ctx* ctx)
{
	if (!ctx) return "null context";
	return CIMBAR_FWD(cimbar_hip_last_error);
}

int cimbar_hip_device(const cimbar_hip_ctx* ctx)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_device);
}

int cimbar_hip_decode_frame(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, size_t stride, int should_preprocess, int color_correction, uint8_t* chunks, uint32_t* good_mask)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_decode_frame, rgb, width, height, stride, should_preprocess, color_correction, chunks, good_mask);
}

long long cimbar_hip_decode_frame_async(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, size_t stride, int should_preprocess, int color_correction, uint8_t* chunks, uint32_t* good_mask)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_decode_frame_async, rgb, width, height, stride, should_preprocess, color_correction, chunks, good_mask);
}

int cimbar_hip_decode_frame_wait(cimbar_hip_ctx* ctx, long long ticket)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_decode_frame_wait, ticket);
}

int64_t cimbar_hip_decode_batch(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction, uint8_t* chunks, uint32_t* masks, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_decode_batch, rgb, n, rgb_mem, should_preprocess, color_correction, chunks, masks, out_mem, hip_stream);
}

int cimbar_hip_decode_batch_pipelined(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int should_preprocess, int color_correction, uint8_t* chunks, uint32_t* masks, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_decode_batch_pipelined, rgb, n, should_preprocess, color_correction, chunks, masks, hip_stream);
}

int cimbar_hip_pipeline_wait(cimbar_hip_ctx* ctx, void* hip_stream, int keep_newest)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_pipeline_wait, hip_stream, keep_newest);
}

int cimbar_hip_pipeline_depth(const cimbar_hip_ctx* ctx)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_pipeline_depth);
}

int64_t cimbar_hip_decode_plain_batch(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction, uint8_t* bytes, uint8_t* block_ok, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_decode_plain_batch, rgb, n, rgb_mem, should_preprocess, color_correction, bytes, block_ok, out_mem, hip_stream);
}

int cimbar_hip_reset_ccm(cimbar_hip_ctx* ctx)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_reset_ccm);
}

int cimbar_hip_get_ccm(cimbar_hip_ctx* ctx, float out9[9])
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_get_ccm, out9);
}

int cimbar_hip_set_ccm(cimbar_hip_ctx* ctx, const float m9[9])
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_set_ccm, m9);
}

int cimbar_hip_set_template(cimbar_hip_ctx* ctx, const uint8_t* rgb_template, int mem)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_set_template, rgb_template, mem);
}

int cimbar_hip_set_erasure_decode(cimbar_hip_ctx* ctx, int sym_distance, int colour_margin, int max_erasures)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_set_erasure_decode, sym_distance, colour_margin, max_erasures);
}

int cimbar_hip_get_erasure_decode(cimbar_hip_ctx* ctx, int* sym_distance, int* colour_margin, int* max_erasures)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_get_erasure_decode, sym_distance, colour_margin, max_erasures);
}

int cimbar_hip_set_colour_erasure_decode(cimbar_hip_ctx* ctx, int colour_margin, int max_erasures)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_set_colour_erasure_decode, colour_margin, max_erasures);
}

int cimbar_hip_get_colour_erasure_decode(cimbar_hip_ctx* ctx, int* colour_margin, int* max_erasures)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_get_colour_erasure_decode, colour_margin, max_erasures);
}

int cimbar_hip_set_relaxed_flood(cimbar_hip_ctx* ctx, int threshold, int fallback)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_set_relaxed_flood, threshold, fallback);
}

int cimbar_hip_get_relaxed_flood(cimbar_hip_ctx* ctx, int* threshold, int* fallback)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_get_relaxed_flood, threshold, fallback);
}

int cimbar_hip_relaxed_flood_stats(cimbar_hip_ctx* ctx, int64_t out[4])
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_relaxed_flood_stats, out);
}

int cimbar_hip_set_group_colour_vote(cimbar_hip_ctx* ctx, int on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_set_group_colour_vote, on);
}

int cimbar_hip_get_group_colour_vote(cimbar_hip_ctx* ctx, int* on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_get_group_colour_vote, on);
}

int cimbar_hip_set_once_rescue(cimbar_hip_ctx* ctx, int on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_set_once_rescue, on);
}

int cimbar_hip_get_once_rescue(cimbar_hip_ctx* ctx, int* on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_get_once_rescue, on);
}

int cimbar_hip_set_once_tear_skip(cimbar_hip_ctx* ctx, int axis, int line_permille, int min_side)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_set_once_tear_skip, axis, line_permille, min_side);
}

int cimbar_hip_get_once_tear_skip(cimbar_hip_ctx* ctx, int* axis, int* line_permille, int* min_side)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_get_once_tear_skip, axis, line_permille, min_side);
}

int cimbar_hip_set_once_tear_salvage(cimbar_hip_ctx* ctx, int on, int guard_lines)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_set_once_tear_salvage, on, guard_lines);
}

int cimbar_hip_get_once_tear_salvage(cimbar_hip_ctx* ctx, int* on, int* guard_lines)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_get_once_tear_salvage, on, guard_lines);
}

int cimbar_hip_set_stream_colour_vote(cimbar_hip_ctx* ctx, int on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_set_stream_colour_vote, on);
}

int cimbar_hip_get_stream_colour_vote(cimbar_hip_ctx* ctx, int* on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_get_stream_colour_vote, on);
}

int cimbar_hip_rs_decode_erasures(cimbar_hip_ctx* ctx, const uint8_t* blocks, int n, const uint8_t* erasures, const uint8_t* counts, int mem,
                                  uint8_t* msgs, int8_t* status, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_rs_decode_erasures, blocks, n, erasures, counts, mem, msgs, status, hip_stream);
}

int64_t cimbar_hip_decode_batch_combined(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                         const int* groups_in, int min_agree_permille, int max_group, uint8_t* chunks, uint32_t* masks,
                                         int* groups_out, uint8_t* gchunks, uint32_t* gmasks, int* n_groups, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_decode_batch_combined, rgb, n, rgb_mem, should_preprocess, color_correction, groups_in, min_agree_permille, max_group,
	                  chunks, masks, groups_out, gchunks, gmasks, n_groups, out_mem, hip_stream);
}

int64_t cimbar_hip_scan_extract_decode_batch_combined_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n,
                                                          int img_mem, int preprocess, int color_correction, const int* groups_in,
                                                          int min_agree_permille, int max_group, uint8_t* chunks, uint32_t* masks, int* status,
                                                          int* groups_out, uint8_t* gchunks, uint32_t* gmasks, int* n_groups, int out_mem,
                                                          void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_scan_extract_decode_batch_combined_fmt, img, width, height, format, n, img_mem, preprocess, color_correction, groups_in,
	                  min_agree_permille, max_group, chunks, masks, status, groups_out, gchunks, gmasks, n_groups, out_mem, hip_stream);
}

int64_t cimbar_hip_decode_batch_combined_stream(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                                int min_agree_permille, int max_group, int flush, uint8_t* chunks, uint32_t* masks, int* groups_out,
                                                uint8_t* gchunks, uint32_t* gmasks, int* gsizes, int* n_groups, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_decode_batch_combined_stream, rgb, n, rgb_mem, should_preprocess, color_correction, min_agree_permille, max_group, flush,
	                  chunks, masks, groups_out, gchunks, gmasks, gsizes, n_groups, out_mem, hip_stream);
}

int64_t cimbar_hip_scan_extract_decode_batch_combined_stream_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format,
                                                                 int n, int img_mem, int preprocess, int color_correction, int min_agree_permille,
                                                                 int max_group, int flush, uint8_t* chunks, uint32_t* masks, int* status,
                                                                 int* groups_out, uint8_t* gchunks, uint32_t* gmasks, int* gsizes, int* n_groups,
                                                                 int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_scan_extract_decode_batch_combined_stream_fmt, img, width, height, format, n, img_mem, preprocess, color_correction,
	                  min_agree_permille, max_group, flush, chunks, masks, status, groups_out, gchunks, gmasks, gsizes, n_groups, out_mem, hip_stream);
}

int64_t cimbar_hip_decode_batch_stitched(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                         int axis, int min_agree_permille, int min_band, uint8_t* chunks, uint32_t* masks, uint8_t* schunks,
                                         uint32_t* smasks, int32_t* tears, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_decode_batch_stitched, rgb, n, rgb_mem, should_preprocess, color_correction, axis, min_agree_permille, min_band, chunks,
	                  masks, schunks, smasks, tears, out_mem, hip_stream);
}

int64_t cimbar_hip_scan_extract_decode_batch_stitched_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n,
                                                          int img_mem, int preprocess, int color_correction, int axis, int min_agree_permille,
                                                          int min_band, uint8_t* chunks, uint32_t* masks, int* status, uint8_t* schunks,
                                                          uint32_t* smasks, int32_t* tears, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_scan_extract_decode_batch_stitched_fmt, img, width, height, format, n, img_mem, preprocess, color_correction, axis,
	                  min_agree_permille, min_band, chunks, masks, status, schunks, smasks, tears, out_mem, hip_stream);
}

int64_t cimbar_hip_decode_batch_stitched_stream(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                                int axis, int min_agree_permille, int min_band, uint8_t* chunks, uint32_t* masks, uint8_t* schunks,
                                                uint32_t* smasks, int32_t* tears, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_decode_batch_stitched_stream, rgb, n, rgb_mem, should_preprocess, color_correction, axis, min_agree_permille, min_band,
	                  chunks, masks, schunks, smasks, tears, out_mem, hip_stream);
}

int64_t cimbar_hip_scan_extract_decode_batch_stitched_stream_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format,
                                                                 int n, int img_mem, int preprocess, int color_correction, int axis,
                                                                 int min_agree_permille, int min_band, uint8_t* chunks, uint32_t* masks, int* status,
                                                                 uint8_t* schunks, uint32_t* smasks, int32_t* tears, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_scan_extract_decode_batch_stitched_stream_fmt, img, width, height, format, n, img_mem, preprocess, color_correction,
	                  axis, min_agree_permille, min_band, chunks, masks, status, schunks, smasks, tears, out_mem, hip_stream);
}

int64_t cimbar_hip_decode_batch_once(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                     int min_agree_permille, int max_run, uint8_t* chunks, uint32_t* masks, int* runs_out, int* roles,
                                     uint8_t* rchunks, uint32_t* rmasks, int* n_runs, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_decode_batch_once, rgb, n, rgb_mem, should_preprocess, color_correction, min_agree_permille, max_run, chunks, masks,
	                  runs_out, roles, rchunks, rmasks, n_runs, out_mem, hip_stream);
}

int64_t cimbar_hip_scan_extract_decode_batch_once_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n,
                                                      int img_mem, int preprocess, int color_correction, int min_agree_permille, int max_run,
                                                      uint8_t* chunks, uint32_t* masks, int* status, int* runs_out, int* roles, uint8_t* rchunks,
                                                      uint32_t* rmasks, int* n_runs, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_scan_extract_decode_batch_once_fmt, img, width, height, format, n, img_mem, preprocess, color_correction,
	                  min_agree_permille, max_run, chunks, masks, status, runs_out, roles, rchunks, rmasks, n_runs, out_mem, hip_stream);
}

int64_t cimbar_hip_decode_batch_once_stream(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                            int min_agree_permille, int max_run, uint8_t* chunks, uint32_t* masks, int* runs_out, int* roles,
                                            uint8_t* rchunks, uint32_t* rmasks, int* n_runs, int* continued, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_decode_batch_once_stream, rgb, n, rgb_mem, should_preprocess, color_correction, min_agree_permille, max_run, chunks,
	                  masks, runs_out, roles, rchunks, rmasks, n_runs, continued, out_mem, hip_stream);
}

int64_t cimbar_hip_scan_extract_decode_batch_once_stream_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n,
                                                             int img_mem, int preprocess, int color_correction, int min_agree_permille, int max_run,
                                                             uint8_t* chunks, uint32_t* masks, int* status, int* runs_out, int* roles,
                                                             uint8_t* rchunks, uint32_t* rmasks, int* n_runs, int* continued, int out_mem,
                                                             void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_scan_extract_decode_batch_once_stream_fmt, img, width, height, format, n, img_mem, preprocess, color_correction,
	                  min_agree_permille, max_run, chunks, masks, status, runs_out, roles, rchunks, rmasks, n_runs, continued, out_mem, hip_stream);
}

int cimbar_hip_once_stream_reset(cimbar_hip_ctx* ctx)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_once_stream_reset);
}

int cimbar_hip_stitch_stream_reset(cimbar_hip_ctx* ctx)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_stitch_stream_reset);
}

int cimbar_hip_set_stitch_strips(cimbar_hip_ctx* ctx, int strips)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_set_stitch_strips, strips);
}

int cimbar_hip_get_stitch_strips(cimbar_hip_ctx* ctx, int* strips)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_get_stitch_strips, strips);
}

int cimbar_hip_set_stitch_erasure(cimbar_hip_ctx* ctx, int on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_set_stitch_erasure, on);
}

int cimbar_hip_get_stitch_erasure(cimbar_hip_ctx* ctx, int* on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_get_stitch_erasure, on);
}

int cimbar_hip_combine_stream_reset(cimbar_hip_ctx* ctx)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_combine_stream_reset);
}

int cimbar_hip_encode_batch(cimbar_hip_ctx* ctx, const uint8_t* payload, int n, int payload_mem, uint8_t* rgb_out, int rgb_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_encode_batch, payload, n, payload_mem, rgb_out, rgb_mem, hip_stream);
}

int cimbar_hip_scan_preprocess(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int n, int rgb_mem, uint8_t* binary, int* thresholds, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_scan_preprocess, rgb, width, height, n, rgb_mem, binary, thresholds, out_mem, hip_stream);
}

int cimbar_hip_deskew_batch(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int n, int rgb_mem, const float* corners, uint8_t* frames, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_deskew_batch, rgb, width, height, n, rgb_mem, corners, frames, out_mem, hip_stream);
}

int cimbar_hip_extract_batch(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int n, int rgb_mem, uint8_t* frames, int* status, float* corners, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_extract_batch, rgb, width, height, n, rgb_mem, frames, status, corners, out_mem, hip_stream);
}

int64_t cimbar_hip_scan_extract_decode_batch(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int n, int rgb_mem, int preprocess, int color_correction, uint8_t* chunks, uint32_t* masks, int* status, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_scan_extract_decode_batch, rgb, width, height, n, rgb_mem, preprocess, color_correction, chunks, masks, status, out_mem, hip_stream);
}

// the same four with the capture's pixel format (the `format` argument of cimbard_scan_extract_decode, cimbar_recv_js.h:17)
size_t cimbar_hip_capture_bytes(unsigned width, unsigned height, int format)
{
	const int fmt = m68::capture_format(format);
	if (!m68::capture_dims_ok(width, height, fmt)) return 0;
	return m68::capture_bytes(width, height, fmt);
}

int cimbar_hip_scan_preprocess_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n, int img_mem, uint8_t* binary, int* thresholds, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_scan_preprocess_fmt, img, width, height, format, n, img_mem, binary, thresholds, out_mem, hip_stream);
}

int cimbar_hip_deskew_batch_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n, int img_mem, const float* corners, uint8_t* frames, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_deskew_batch_fmt, img, width, height, format, n, img_mem, corners, frames, out_mem, hip_stream);
}

int cimbar_hip_extract_batch_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n, int img_mem, uint8_t* frames, int* status, float* corners, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_extract_batch_fmt, img, width, height, format, n, img_mem, frames, status, corners, out_mem, hip_stream);
}

int64_t cimbar_hip_scan_extract_decode_batch_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n, int img_mem, int preprocess, int color_correction, uint8_t* chunks, uint32_t* masks, int* status, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_scan_extract_decode_batch_fmt, img, width, height, format, n, img_mem, preprocess, color_correction, chunks, masks, status, out_mem, hip_stream);
}

int cimbar_hip_undistort_calibrate_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n, int img_mem, int* ok, double* k1, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_undistort_calibrate_fmt, img, width, height, format, n, img_mem, ok, k1, hip_stream);
}

int cimbar_hip_undistort_batch_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n, int img_mem, const double* params, uint8_t* out_rgb, int out_mem, int* ok, double* k1_out, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_undistort_batch_fmt, img, width, height, format, n, img_mem, params, out_rgb, out_mem, ok, k1_out, hip_stream);
}

int64_t cimbar_hip_scan_undistort_extract_decode_batch_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n, int img_mem, int preprocess, int color_correction, uint8_t* chunks, uint32_t* masks, int* status, int* undistort_ok, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_scan_undistort_extract_decode_batch_fmt, img, width, height, format, n, img_mem, preprocess, color_correction, chunks, masks, status, undistort_ok, out_mem, hip_stream);
}

int64_t cimbar_hip_tap(cimbar_hip_ctx* ctx, int what, void* out, size_t out_bytes)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_tap, what, out, out_bytes);
}

int cimbar_hip_enable_timing(cimbar_hip_ctx* ctx, int on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_enable_timing, on);
}

int cimbar_hip_stage_times(cimbar_hip_ctx* ctx, const char** names, float* ms, int max)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_stage_times, names, ms, max);
}

int64_t cimbar_hip_deliver_chunks(cimbar_hip_ctx* ctx, const uint8_t* chunks, const uint32_t* masks, int n, int in_mem, unsigned flags, uint8_t* packed, int32_t* src, int32_t* count, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return deliver::deliver_chunks(delivery_view(ctx), chunks, masks, n, in_mem, flags, packed, src, count, out_mem, hip_stream);
}

int cimbar_hip_delivery_reset(cimbar_hip_ctx* ctx, int capacity_log2)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return deliver::delivery_reset(delivery_view(ctx), capacity_log2);
}

int cimbar_hip_delivery_stats(cimbar_hip_ctx* ctx, int64_t* remembered, int64_t* capacity, int* overflowed)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return deliver::delivery_stats(delivery_view(ctx), remembered, capacity, overflowed);
}

int cimbar_hip_geometry(const cimbar_hip_ctx* ctx, int32_t out[CIMBAR_HIP_GEOMETRY_WORDS])
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return CIMBAR_FWD(cimbar_hip_geometry, out);
}

}  // extern "C"
