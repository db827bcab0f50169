// host.hip.inc -- part of cimbar_hip.hip (one translation unit; included at file scope after the kernels).
// host side: context, tables, launch structure, C ABI
// ================================================================================================ host side / C ABI
// what the stream calls of the group decode keep between calls (combine.hip.inc, "the stream calls"): the carry store, its device-side
// counters and the event that orders one stream call behind the one before. Nothing of it exists until the first stream call.
struct CombineStream {
	DevBuf<uint8_t> symbols, colors, chunks; DevBuf<uint32_t> plane, flood, masks; DevBuf<int8_t> drift;
	DevBuf<uint32_t> weights;                 // [CARRY_SLOTS][CS_WEIGHTS] the colour vote's weights of the carried members; allocated by the first stream call with cimbar_hip_set_stream_colour_vote on
	DevBuf<int> words;                        // [0] occupied slots, [1] members of the open group of the call in flight (k_group_walk_stream -> k_group_carry)
	DevBuf<int> gsizes;                       // staging for host-memory gsizes, n + 1 ints, grown on demand
	Event ev_last;                            // behind the last stream call's work: the next one, on whatever stream, starts after it
	bool used = false;
	int min_agree = 0, max_group = 0;         // fixed by the first stream call after create / reset (0: not yet)
	int vote = 0;                             // ... and so is cimbar_hip_set_stream_colour_vote's value (read while max_group != 0)
	CarryStore store() const { return CarryStore{symbols, colors, plane, drift, flood, chunks, masks, words, weights}; }
};

// what the stream calls of torn-capture stitching keep between calls (stitch.hip.inc, "the stream calls"): the last capture's decided cells
// in two slots used in turn, one usable word per slot and the event that orders one stream call behind the one before. Nothing of it exists
// until the first stitched-stream call.
struct StitchStream {
	DevBuf<uint8_t> symbols, colors;          // [2][SS_CELLS]
	DevBuf<uint32_t> usable;                  // [2]
	Event ev_last;                            // behind the last stitched-stream call's work: the next one, on whatever stream, starts after it
	bool used = false;                        // ev_last has been recorded
	bool carried = false;                     // slot `cur` holds the last capture of a stream call (CIMBAR_HIP_TAP_STITCH_CARRY describes it)
	int cur = 0;                              // the slot the next call reads
	StitchCarry carry() const { return StitchCarry{symbols, colors, usable, cur}; }
};

// what the once-stream calls of repeat-capture skipping keep between calls (repeat.hip.inc, "runs across calls"): the last capture's
// signature, words and run row in two slots used in turn, the words of the call in flight and the event that orders one once-stream call
// behind the one before. Nothing of it exists until the first once-stream call.
struct OnceStream {
	DevBuf<uint8_t> sig, row;                 // [2][RP_CARRY_SIG], [2][RP_CARRY_ROW]
	DevBuf<uint32_t> words;                   // [2][RP_CARRY_WORDS]
	DevBuf<int> cw; PinnedBuf<int> h_cw;      // [RP_CALL_WORDS] of the call in flight, and where their read-backs land
	Event ev_last;                            // behind the last once-stream call's work: the next one, on whatever stream, starts after it
	bool used = false;                        // ev_last has been recorded
	bool carried = false;                     // slot `cur` holds the last capture of a once-stream call (CIMBAR_HIP_TAP_REPEAT_CARRY describes it)
	int cur = 0;                              // the slot the next call reads
	RepeatCarry carry() const { return RepeatCarry{sig, words, row, cur}; }
};

struct cimbar_hip_ctx {
	int mode_tag = MODE_VAL;                  // FIRST member: api.hip.inc reads it through the opaque pointer to pick the namespace
	int device = 0;
	// Everything below that owns something (devbuf.hip.inc) frees it in its destructor, after the body of ~cimbar_hip_ctx() at the end of this struct.
	Stream stream;
	Stream stream2;                           // second half of a batch's tail kernels (see enqueue)
	Event ev_k1, ev_join, ev_mid[CHAIN_PARTS_MAX];
	int tail_split = 1, tail_parts = 2;
	PinnedBuf<uint32_t> h_flagged;    // written by k_count_flagged at the end of every ordinary batch: [0] frames that left the parallel path, [1] frames of that batch,
	                                  // [2] frames the exact replay (or, with the relaxed flood on, k_flood_rounds) had to take.
	int er_sym = 0, er_col = -1, er_max = -1;   // cimbar_hip_set_erasure_decode: off while er_sym <= 0 (k_erasure_frame is then never launched)
	int ec_margin = 0, ec_max = -1;             // cimbar_hip_set_colour_erasure_decode: off while ec_margin <= 0 (k_colour_erasure_frame is then never launched)
	bool cm_valid = false;                      // the last batch ran the colour retry (CIMBAR_HIP_TAP_COLOUR_MARGIN describes it)
	DevBuf<uint8_t> d_er_buf;                   // cimbar_hip_rs_decode_erasures' staging for host-memory calls (grown on demand)
	std::unique_ptr<deliver::State> delivery;   // cimbar_hip_deliver_chunks' scratch and remembered headers (deliver.hip.inc): nothing of it exists until the first call
	// the group decode (cimbar_hip_decode_batch_combined / _scan_extract_decode_batch_combined_fmt, combine.hip.inc): per capture slot, grown on demand
	bool grp_valid = false;                     // the last batch was a combined one (the group taps describe it)
	DevBuf<uint8_t> d_gsym, d_gcol; DevBuf<uint16_t> d_gmargin; DevBuf<uint8_t> d_grs_ok;   // [n][NCELLS], [n][ALL_BLOCKS]
	DevBuf<uint32_t> d_gagree, d_gdisp; DevBuf<int> d_groups, d_gmem, d_gcount, d_groups_in;
	DevBuf<int> d_ngroups;                      // 1 int
	DevBuf<uint8_t> d_gchunks; DevBuf<uint32_t> d_gmasks;   // staging for host-memory group outputs
	int gcv_on = 0;                             // cimbar_hip_set_group_colour_vote: off unless set (k_group_colour / k_group_colour_retry are then never launched)
	int sgv_on = 0;                             // cimbar_hip_set_stream_colour_vote: the same for the stream calls (k_group_colour_stream / k_group_carry_weights / k_group_colour_retry)
	bool gcv_valid = false;                     // the last batch was a combined one that ran the vote (CIMBAR_HIP_TAP_GROUP_COLOUR_* describe it)
	int gcv_stream_n = -1;                      // ... >= 0: a stream call of that many captures (CIMBAR_HIP_TAP_STREAM_CARRY_WEIGHTS describes its carry store)
	DevBuf<uint32_t> d_gcm, d_gcw;              // the vote's margins [groups][NCELLS] and member weights [captures][NCELLS]; allocated by the first combined call with its setting on
	std::unique_ptr<CombineStream> cstream;     // cimbar_hip_decode_batch_combined_stream / _scan_extract_decode_batch_combined_stream_fmt
	// torn-capture stitching (cimbar_hip_decode_batch_stitched / _scan_extract_decode_batch_stitched_fmt, stitch.hip.inc): per pair slot, grown on demand
	int stitch_n = 0, stitch_axis = 0;          // the last batch was a stitched one of stitch_n captures (> 0: the stitch taps describe it)
	int stitch_rows = 0;                        // ... and reported that many pair rows: stitch_n - 1, a stream call stitch_n
	DevBuf<uint8_t> d_ssym, d_scol, d_srs_ok;   // [2 rows][NCELLS], [2 rows][ALL_BLOCKS]
	DevBuf<uint32_t> d_slive; DevBuf<int32_t> d_stears; DevBuf<uint16_t> d_slines; DevBuf<int> d_sslots;   // [2 rows], [rows][4], [rows][L], 1 int
	std::unique_ptr<StitchStream> sstream;      // cimbar_hip_decode_batch_stitched_stream / _scan_extract_decode_batch_stitched_stream_fmt
	int stitch_strips = 1;                      // cimbar_hip_set_stitch_strips: 1 = whole lines (k_stitch_pairs), 2..8 = k_stitch_pairs_strips
	int stitch_S = 1;                           // the strips of the last stitched batch (> 1: the strip taps describe it)
	DevBuf<int32_t> d_sstrips; DevBuf<uint16_t> d_sstrip_lines;   // [rows][S][4], [rows][S][L]: allocated by the first stitched call with strips > 1
	DevBuf<uint8_t> d_schunks; DevBuf<uint32_t> d_smasks;   // staging for host-memory stitch outputs
	// the stitched decode's erasure retry (cimbar_hip_set_stitch_erasure, stitch.hip.inc S3 / S4): nothing of it exists until a plain stitched call runs with it on
	int stitch_er = 0;                          // the setting
	int stitch_er_ran = 0;                      // the last stitched batch: bit 0 = S3 ran, bit 1 = S4 ran (CIMBAR_HIP_TAP_STITCH_DISTANCE / _COLOUR_MARGIN describe it)
	DevBuf<uint8_t> d_sdist; DevBuf<uint32_t> d_smargin, d_sworked;   // [2 rows][NCELLS] each; [2][2 rows] "worked on" words, S3's then S4's
	// repeat-capture skipping (cimbar_hip_decode_batch_once / _scan_extract_decode_batch_once_fmt, repeat.hip.inc): per capture, grown on demand;
	// the gathered frames and their results are sized by the longer of a call's two lists
	int rp_n = 0;                               // the last once-call had that many captures (> 0: the repeat taps describe it)
	bool rp_stream = false;                     // ... and was a once-stream call (its agreement has rp_n entries, entry 0 against the carry)
	std::unique_ptr<OnceStream> ostream;        // cimbar_hip_decode_batch_once_stream / _scan_extract_decode_batch_once_stream_fmt
	DevBuf<ushort4> d_rp_sums; DevBuf<uint8_t> d_rp_sig; DevBuf<uint32_t> d_rp_agree;   // [n][NCELLS], [n][NCELLS], [n]
	DevBuf<int> d_rp_runs, d_rp_mem, d_rp_count, d_rp_roles, d_rp_list, d_rp_sel;        // [n], [n][GMAX], [n], [n], [2][n] lists 1 and 2, [list] scan status
	DevBuf<int> d_rp_words; PinnedBuf<int> h_rp_words;                                   // [0] runs = the length of list 1, [1] the length of list 2
	DevBuf<uint8_t> d_rp_frames, d_rp_chunks; DevBuf<uint32_t> d_rp_masks;               // [list] gathered frames and what their decode delivered
	DevBuf<uint8_t> d_rp_rchunks; DevBuf<uint32_t> d_rp_rmasks;                          // staging for host-memory run outputs
	// run rescue (cimbar_hip_set_once_rescue, repeat.hip.inc "run rescue"): nothing of it exists until a plain once-call with the setting on needs it.
	// The rescue's group scratch is the combined calls' (d_gsym .. d_gmasks above), sized by the rescue slots.
	int rs_on = 0;                              // the setting
	int rs_state = 0;                           // the last once-call: 0 = a stream call or the setting off, 1 = on and nothing launched, 2 = the rescue kernels ran
	int rs_slots = 0;                           // ... over that many slots (the host's bound on the qualifying runs)
	DevBuf<uint8_t> d_rs_symbols, d_rs_colors; DevBuf<int8_t> d_rs_drift; DevBuf<uint32_t> d_rs_plane, d_rs_flood;   // the store: [slots] x CS_CELLS, CS_CELLS, CS_DRIFT, CS_PLANE, 1
	DevBuf<int> d_rs_run, d_rs_map, d_rs_count; DevBuf<int32_t> d_rs_tap;                // [slots] the slot's run, [n] where a member's cells are, 1 int, [n] CIMBAR_HIP_TAP_ONCE_RESCUE
	// tear skipping (cimbar_hip_set_once_tear_skip, repeat.hip.inc "tear skipping"): nothing of it exists until a plain once-call with the setting on
	int rt_axis = -1, rt_line = RT_LINE_DEFAULT, rt_side = RT_SIDE_DEFAULT;   // the setting, resolved; axis -1 = off
	bool rt_state = false;                      // the last once-call was a plain one with the setting on (CIMBAR_HIP_TAP_ONCE_TEAR describes it)
	DevBuf<int32_t> d_rt_tap; DevBuf<int> d_rt_pos, d_rt_words; PinnedBuf<int> h_rt_words;   // [n][4] the records, [n] a run's place in list 1, {|list 1|, |list 2|} and their mirror
	// tear salvage (cimbar_hip_set_once_tear_salvage, repeat.hip.inc "tear salvage"): nothing of it exists until a plain once-call in which it is effective
	int sv_on = 0, sv_guard = RV_GUARD_DEFAULT; // the setting, resolved
	bool sv_state = false;                      // the last once-call was a plain one in which the setting was effective (CIMBAR_HIP_TAP_ONCE_SALVAGE describes it)
	DevBuf<int32_t> d_sv_part; DevBuf<int> d_sv_full;   // [slots][8] the slots' partials, [slots] the full members of a tried slot
	int wave_adapt = 1;               // CIMBAR_HIP_FLOOD_WAVE_ADAPT=0: run k_flood_wave in front of every exact replay, whatever it achieved before
	bool wave_ran = false;            // k_flood_wave ran in the batch h_flagged describes
	int wave_skip_left = 0;           // batches that still go straight to the exact replay (see enqueue)
	                                  // The NEXT ordinary call reads it without waiting (a stale value only costs the heuristic): a stream of distorted frames runs un-split too
	std::string err;
	Tables tb{};                      // what the kernels take by value: filled by build_tables from the owners beside it
	DevBuf<ushort2> tb_cell_xy; DevBuf<uint16_t> tb_stream_cell, tb_cell_grid, tb_ccm_grid; DevBuf<int16_t> tb_grid_cell, tb_cand;
	DevBuf<uint8_t> tb_stitch_line;  // [2][NCELLS] the grid row and the grid column of every cell (k_stitch_pairs)
	DevBuf<uint16_t> tb_stitch_width;  // [2][STITCH_SMAX][STITCH_SMAX][128] width(l, j) by axis, S - 1, strip and line (k_stitch_pairs_strips)
	uint64_t tile_hashes[16] = {};   // as computed at create (also in c_tile)
	int last_n = 0;
	int scan_n = 0;                             // captures of the last anchor search (CIMBAR_HIP_TAP_SCAN_PATH describes it)
	unsigned scan_w = 0, scan_h = 0;            // ... and their size (CIMBAR_HIP_TAP_SCAN_GRAY: scan_n planes of scan_w x scan_h in d_ex_gray)
	DevBuf<uint8_t> d_rgb;            // staging for host-resident input
	// the intermediates of a batch (grown on demand). A context has `pipe_depth` sets of them and as many streams: the pipelined entry point steps to the
	// next set with every batch, so that several batches are in flight at once; every other call uses the set the newest batch used (cur())
	static constexpr int MAXP = 4;
	struct ScratchSet {
		int cap = 0;                      // frames the set holds
		DevBuf<uint32_t> d_plane, d_cellmean;
		DevBuf<uint8_t> d_symbols, d_colors;
		DevBuf<int8_t> d_drift;
		DevBuf<uint32_t> d_flood;         // [cap] frame flags, then [cap] what k_flood_wave made of the frame (CIMBAR_HIP_TAP_FLOOD_INFO), then [cap] what k_flood_rounds did
		                                  // (CIMBAR_HIP_TAP_FLOOD_ROUNDS); zeroed when it grows
		DevBuf<uint8_t> d_rs_ok;
		DevBuf<FrameState> d_states;
		DevBuf<float> d_ccm_frames, d_ccm_used;
		DevBuf<uint32_t> d_cmargin;       // the colour retry's margins [cm_cap][NCELLS], then its per-frame "worked on" words [cm_cap]; allocated once the setting is on
		int cm_cap = 0;
	} sets[MAXP];
	int pipe_depth = 3;               // batches in flight (CIMBAR_HIP_PIPE_DEPTH): 3 measured best once every step reads HBM (4 distinct input batches): 0.81 vs 0.85 ms at 4
#ifdef CIMBAR_PROBES
	int dbg_skip = 0;                 // CIMBAR_HIP_DEBUG_SKIP (probe builds only, -DCIMBAR_PROBES: python -m libcimbar_amd.build --probes): bit mask of chain kernels NOT launched -- timing experiments, results are then wrong
#else
	static constexpr int dbg_skip = 0; // the product library cannot drop a kernel: the switch and the k_rs<.., NOSYND> instances only exist in a -DCIMBAR_PROBES build
#endif
	int pipe_set = 0;                 // the set in use
	ScratchSet& cur() { return sets[pipe_set]; }
	bool pipe_used[MAXP] = {};
	Stream pstream_own[MAXP];         // the streams the pipeline needs beyond stream / stream2 ([0], [1] stay empty)
	hipStream_t pstream[MAXP] = {};   // set k's stream: stream, stream2, then pstream_own[k]
	Event ev_pk1[MAXP], ev_pdone[MAXP];
	Event ev_pgather[MAXP];            // cimbar_hip_pipeline_gather: "the exchange behind this set's batch is over" (an event of its own: the NEXT batch's colour pass waits for
	bool pipe_gathered[MAXP] = {};     // ev_pdone only -- the carry-over must not wait for other ranks). pipeline_wait waits for both where a gather was issued
	// one frame per call, up to pipe_depth of them in flight (cimbar_hip_decode_frame_async / _wait): slot s rides on scratch set s and stream s of the
	// pipeline above -- frame k+1's host-to-device copy runs on another queue than frame k's kernels, which is the whole point
	struct FrameSlot {
		DevBuf<uint8_t> d_rgb;           // the frame on the device
		DevBuf<uint8_t> d_out;           // its chunks [FRAME_OUT_STRIDE] + mask [4]
		PinnedBuf<uint8_t> h_out;        // where the one device-to-host copy lands
		PinnedBuf<uint8_t> h_in;         // staging for frames that arrive in pageable memory (allocated when one does)
		Event done;
		uint8_t* user_chunks = nullptr; uint32_t* user_mask = nullptr;
		long long ticket = -1;           // >= 0: in flight
	} fslot[MAXP];
	long long frame_tickets = 0;
	int k1_tall = -1;                 // CIMBAR_HIP_K1_STRIPS=short|tall|auto: which instance of the plain threshold kernel a launch takes (auto: tall inside the pipelined loop for batches of K1_TALL_MIN frames and more)
	int k1_lds_pad = 0;               // CIMBAR_HIP_K1_LDS_PAD: dynamic LDS bytes reserved per K1 workgroup (an occupancy cap for experiments: 30000 -> two workgroups per CU)
	size_t warp_scratch = (size_t)4 << 30;   // CIMBAR_HIP_WARP_SCRATCH_MB: what the two-pass warp may hold of converted captures at a time (it goes through a batch in passes of that many captures, at most WARP_CHUNK)
	int warp_twopass = 1;             // CIMBAR_HIP_WARP_TWOPASS=0: YUV captures (12 / 21 / 420 / 422 / 4221) are converted inside the warp kernel, tap by tap, instead of once per source pixel ahead of it
	DevBuf<int4> d_ex_box;            // ... and the box of every capture (k_roi_boxes)
	DevBuf<uint8_t> d_ex_rgb;         // ... the capture-shaped RGB8 scratch of that conversion, WARP_CHUNK captures at a time
	int frame_stage = 0;              // CIMBAR_HIP_FRAME_STAGE=1: pageable frames go through the context's own page-locked staging instead of the runtime's
	int frame_zerocopy = 1;           // CIMBAR_HIP_FRAME_ZEROCOPY=0: chunks + mask go to device memory and come back with a copy, instead of being written to page-locked host memory by the kernels
	int frame_copystream = 0;         // CIMBAR_HIP_FRAME_COPYSTREAM=1: every frame's host-to-device copy on one stream of its own (never queued behind another frame's copy back)
	Stream fcopy;
	Event ev_fcopy[MAXP];
	struct FrameResult { long long ticket = -1; int rc = 0; } fresult[16];   // return values of frames that are complete but not yet asked for
	DevBuf<float> d_carry;            // 10 floats
	DevBuf<uint8_t> d_template;       // encode half: empty frame (background, anchors, guides)
	DevBuf<uint8_t> d_gen_log;        // encode half: logs of the 30 low generator coefficients
	DevBuf<uint8_t> d_payload;        // encode half: staging for host-resident payload
	DevBuf<uint8_t> d_chunks;         // staging for host-resident output: shared by every scratch set, so it grows on its own
	DevBuf<uint32_t> d_masks;
	// extractor stage (scan_preprocess / deskew_batch): staging + small per-frame state
	DevBuf<uint8_t> d_ex_in;
	DevBuf<uint8_t> d_ex_out;
	DevBuf<uint32_t> d_ex_hist; DevBuf<int> d_ex_thr; DevBuf<double> d_ex_minv;
	DevBuf<uint8_t> d_ex_gray;        // blurred gray captures (what the anchor search reads)
	DevBuf<uint8_t> d_ex_frames;      // deskewed frames of scan_extract_decode
	DevBuf<uint32_t> d_scan_hits; DevBuf<int> d_scan_nhits; DevBuf<ScanResult> d_scan_res;
	DevBuf<ScanAnchor> d_scan_serial;   // scratch lists of k_scan_serial (captures whose anchor search overflowed the fast kernels' lists)
	DevBuf<int> d_scan_offs, d_scan_ovf; DevBuf<ScanConf> d_scan_conf; DevBuf<ScanStage> d_scan_stage;   // stage[0..n) primary, [n..2n) bottom-right
	PinnedBuf<double> h_ex_minv;      // staging for the warp matrices (an async copy must not read a pageable temporary)
	Event ev_ex_minv;                 // the last copy out of h_ex_minv
	// lens undistortion (cimbar_hip_undistort_* / cimbar_hip_scan_undistort_extract_decode_batch_fmt): nothing of it exists until one of those is called
	DevBuf<uint8_t> d_ud_img;         // the undistorted RGB8 captures of one group (at most ud_scratch bytes, see undistort_group)
	DevBuf<int> d_ud_ok; DevBuf<double> d_ud_k1; DevBuf<int> d_ud_status;   // per capture of a call
	DevBuf<double> d_ud_xt; PinnedBuf<double> h_ud_xt;   // the column table of U2 (device + page-locked staging)
	Event ev_ud_xt;                   // the last copy out of h_ud_xt
	size_t ud_scratch = (size_t)256 << 20;   // CIMBAR_HIP_UNDISTORT_SCRATCH_MB
	FloodScratch flood{};             // by value into the flood kernels: filled by ensure_flood_areas from the owners beside it
	DevBuf<uint32_t> flood_heap, flood_next; DevBuf<uint8_t> flood_prio;
	int flood_cap = 0;                // spill areas allocated in flood.heap and flood.prio, 0.61 MB of device memory each, grown to what the launches index: one frame -> 0.6 MB,
	                                  // 1 024 frames as one chain -> 620 MB, split or pipelined batches up to 2 048 areas = 1.25 GB (ChainPlan::flood_top)
	// CIMBAR_HIP_TAP_FLOOD_LAUNCH: the exact-replay launches of the last enqueue(), {instance, grid, frames, first frame, area0, counter, flags}
	// each, and the spill areas that enqueue() asked ensure_flood_areas for (host bookkeeping: nothing on the device knows of it)
	int32_t flood_launch[FLOOD_LAUNCH_MAX][7] = {};
	int flood_launch_n = 0, flood_launch_top = 0;
	DevBuf<uint32_t> d_fw_queue;      // k_flood_wave: one work queue of NCELLS entries per resident workgroup
	int flood_verify = 0;             // CIMBAR_HIP_FLOOD_VERIFY=1: every frame k_flood_wave certified is replayed exactly as well and compared (see enqueue)
	DevBuf<uint8_t> d_vsym; DevBuf<int8_t> d_vdrift; DevBuf<uint32_t> d_vflag; int vcap = 0;   // its buffers: saved batch results, [n] flags + [n] differing cells
	DevBuf<unsigned long long> d_vtotals;                                                    // [2] certified frames replayed / frames that differed, since create
	int flood_dense_grid = 2048;      // workgroups of a full-size dense launch (CIMBAR_HIP_FLOOD_DENSE_GRID, <= 2048)
	int flood_dense = -1;             // exact replay at eight frames per CU (k_flood3<HEAP_LDS8, true>): -1 = where a launch has more frames than four per CU hold,
	                                  // 0 = never, 1 = always (CIMBAR_HIP_FLOOD_DENSE)
	int flood_wave = 1;               // run k_flood_wave in front of k_flood (CIMBAR_HIP_FLOOD_WAVE=0 turns it off: exact replay for every flagged frame)
	// the relaxed flood (cimbar_hip_set_relaxed_flood, k2d_floodrounds.hip.inc): off while rf_threshold < 0 -- enqueue() then launches what it always did
	int rf_threshold = -1, rf_fallback = 0;
	int rf_grid = FR_GRID;            // workgroups of k_flood_rounds (CIMBAR_HIP_ROUNDS_GRID lowers it: a workgroup then walks several frames)
	bool rf_valid = false;            // the last batch ran with the setting on (CIMBAR_HIP_TAP_FLOOD_ROUNDS describes it)
	DevBuf<unsigned long long> d_rf_stats;   // [4] cimbar_hip_relaxed_flood_stats; allocated by the setter
	// timing
	bool timing = false;
	static constexpr int NSTAGE = 8;
	Event ev[NSTAGE + 1];
	float stage_ms[NSTAGE] = {};

	// (also what the early returns of cimbar_hip_create run: whatever exists by then is freed by the members, after this body)
	~cimbar_hip_ctx()
	{
		(void)hipSetDevice(device);
		// frames started with cimbar_hip_decode_frame_async and never waited for still have kernels writing into the context's page-locked buffers
		(void)hipDeviceSynchronize();
		if (flood_verify && d_vtotals) {
			unsigned long long t[2] = {0, 0};
			if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(t, d_vtotals, sizeof t, hipMemcpyDeviceToHost) == hipSuccess)
				std::fprintf(stderr, "cimbar_hip: CIMBAR_HIP_FLOOD_VERIFY (mode %d): %llu certified frames replayed exactly, %llu differed\n", MODE_VAL, t[0], t[1]);
		}
	}
};

namespace {

const char* const STAGE_NAMES[cimbar_hip_ctx::NSTAGE] = {"threshold", "symbols", "flood", "rs_symbols", "frame_mid", "colors", "rs_colors", "frame_end"};

#define HIPCHK(call)                                                                                      \
	do {                                                                                                  \
		hipError_t e__ = (call);                                                                          \
		if (e__ != hipSuccess) {                                                                          \
			ctx->err = std::string(#call) + ": " + hipGetErrorString(e__);                                \
			return CIMBAR_HIP_EHIP;                                                                       \
		}                                                                                                 \
	} while (0)

void host_cell_positions(std::vector<ushort2>& xy)
{
	// CellPositions.cpp:5-51 compute_linear for Conf8x8
	xy.resize(NCELLS);
	int n = 0;
	for (int i = 0; i < TOP_CELLS; ++i, ++n) xy[n] = make_ushort2((i % TOP_W) * PITCH + PITCH * MARKER + OFFSET, (i / TOP_W) * PITCH + OFFSET);
	for (int i = 0; i < MID_CELLS; ++i, ++n) xy[n] = make_ushort2((i % DIM_X) * PITCH + OFFSET, (i / DIM_X) * PITCH + MARKER * PITCH + OFFSET);
	for (int i = 0; i < TOP_CELLS; ++i, ++n) xy[n] = make_ushort2((i % TOP_W) * PITCH + PITCH * MARKER + OFFSET, (i / TOP_W) * PITCH + (DIM_Y - MARKER) * PITCH + OFFSET);
}

// AdjacentCellFinder.cpp:16-105, literally (position look-ups included): the index arithmetic there has band-edge quirks
// (e.g. cells 494..499 have no "bottom", 11900..11905 no "top") that the flood order depends on.
struct AdjFinder {
	const std::vector<ushort2>& pos;
	static int in_row_with_margin(int index) { return (index < TOP_CELLS) ? 1 : (index < TOP_CELLS + MID_CELLS ? 0 : 1); }
	int right(int index) const
	{
		if (index < 0 || index >= NCELLS - 1) return -1;
		int next = index + 1;
		if (pos[next].x < pos[index].x) return -1;
		return next;
	}
	int left(int index) const
	{
		int next = index - 1;
		if (next < 0) return -1;
		if (pos[next].x > pos[index].x) return -1;
		return next;
	}
	int bottom(int index) const
	{
		if (index < 0 || index >= NCELLS) return -1;
		int inc = DIM_X;
		if (in_row_with_margin(index)) inc -= MARKER;
		int next = index + inc;
		if (in_row_with_margin(next)) next -= MARKER;
		if (next < 0 || next >= NCELLS) return -1;
		if (pos[next].x != pos[index].x) return -1;
		return next;
	}
	int top(int index) const
	{
		int inc = DIM_X;
		if (in_row_with_margin(index)) inc -= MARKER;
		int next = index - inc;
		if (in_row_with_margin(next)) next += MARKER;
		if (next < 0) return -1;
		if (pos[next].x != pos[index].x) return -1;
		return next;
	}
};

// The 16 symbol tiles of mode B as the reference embeds them (bitmap/4/00.png .. 0f.png in cimb_translator/bitmaps.h, 8x8, foreground
// on white), redrawn here as text: '#' = foreground pixel.
const char* const TILE_BITMAPS[16][8] = {
	{"########", "#######.", "######..", "#####...", "####....", "###.....", "##......", "#......."},   // 0
	{"#.......", "##......", "###.....", "####....", "#####...", "######..", "#######.", "########"},   // 1
	{"########", ".#######", "..######", "...#####", "....####", ".....###", "......##", ".......#"},   // 2
	{".......#", "......##", ".....###", "....####", "...#####", "..######", ".#######", "########"},   // 3
	{"...##...", "...##...", "...##...", "########", "########", "...##...", "...##...", "...##..."},   // 4
	{".##..##.", "###..###", "###..###", "........", "........", "###..###", "###..###", ".##..##."},   // 5
	{"..####..", ".######.", "###..###", "##....##", "##....##", "###..###", ".######.", "..####.."},   // 6
	{"...##...", "...##...", "..####..", "..####..", ".######.", ".######.", "########", "########"},   // 7
	{"##......", "####....", "######..", "########", "########", "######..", "####....", "##......"},   // 8
	{"########", "######..", "####....", "........", "........", "####....", "######..", "########"},   // 9
	{"########", "..######", "....####", "........", "........", "....####", "..######", "########"},   // a
	{"###..###", "###..###", "###..###", "###..###", "##....##", "##....##", "#......#", "#......#"},   // b
	{"#......#", "#......#", "##....##", "##....##", "###..###", "###..###", "###..###", "###..###"},   // c
	{"........", "........", "##....##", "###..###", ".######.", "..####..", "...##...", "........"},   // d
	{"....##..", "...###..", "..###...", ".###....", ".###....", "..###...", "...###..", "....##.."},   // e
	{"...####.", "...####.", "..###...", "..###...", "...###..", "...###..", ".####...", ".####..."},   // f
};

// CimbDecoder::load_tiles (CimbDecoder.cpp:87-99): hash of tile i = average_hash(getTile(4, i, dark, 4 colours)) --
// getTile paints the foreground in colour 0 of the palette on black (Common.cpp:150-171), average_hash (average_hash.h:19-39) takes
// cvtColor(RGB2GRAY) [assumed-OpenCV fixed point, as in K1], thresholds at Cell::mean_grayscale (uint16 sum / count, Cell.h:96-137)
// and packs `p > threshold`, top-left pixel in bit 63. Also builds k_symbols' exact-match slot table and checks it is a perfect hash.
void compute_tile_hashes(uint64_t hashes[16])
{
	const int fg[3] = {0, 255, 0};   // Common.cpp:21-31 getColor4(0)
	for (int t = 0; t < 16; ++t) {
		uint8_t gray[64];
		uint16_t total = 0, count = 0;
		for (int y = 0; y < 8; ++y)
			for (int x = 0; x < 8; ++x, ++count) {
				const bool on = TILE_BITMAPS[t][y][x] == '#';
				const unsigned r = on ? fg[0] : 0, g = on ? fg[1] : 0, b = on ? fg[2] : 0;
				gray[y * 8 + x] = (uint8_t)((r * 9798u + g * 19235u + b * 3735u + (1u << 14)) >> 15);
				total = (uint16_t)(total + gray[y * 8 + x]);
			}
		const uint8_t threshold = (uint8_t)(total / count);
		uint64_t h = 0;
		int bitpos = 63;
		for (int k = 0; k < 64; ++k, --bitpos) h |= (uint64_t)(gray[k] > threshold) << bitpos;
		hashes[t] = h;
	}
}

int build_tile_hashes(cimbar_hip_ctx* ctx, uint64_t hashes[16])
{
	compute_tile_hashes(hashes);
	uint8_t slot[32];
	for (int k = 0; k < 32; ++k) slot[k] = 16;
	for (int t = 0; t < 16; ++t) {
		const uint32_t k = (((uint32_t)hashes[t] ^ (uint32_t)(hashes[t] >> 32)) * TILE_SLOT_MUL) >> 27;
		if (slot[k] != 16) { ctx->err = "build_tile_hashes: the exact-match slot hash collides for these tiles"; return CIMBAR_HIP_EINVAL; }
		slot[k] = (uint8_t)t;
	}
	HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_tile), hashes, sizeof(uint64_t) * 16));
	HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_tile_slot), slot, 32));
	return 0;
}

int build_tables(cimbar_hip_ctx* ctx)
{
	if (int r = build_tile_hashes(ctx, ctx->tile_hashes)) return r;
	std::vector<ushort2> xy;
	host_cell_positions(xy);
	// Interleave.h:8-24 interleave_indices(12400, 155, 2): stream index -> linear cell index
	std::vector<uint16_t> sc;
	sc.reserve(NCELLS);
	const int part_size = NCELLS / 2;
	for (int part = 0; part < NCELLS; part += part_size)
		for (int chunk = 0; chunk < RS_BLOCK; ++chunk)
			for (int i = chunk; i < part_size; i += RS_BLOCK) sc.push_back((uint16_t)(i + part));
	// FloodDecodePositions::update's offer list per cell (FloodDecodePositions.cpp:85-129): adjacents, then both horizons
	std::vector<int16_t> cand((size_t)NCELLS * 12);
	AdjFinder finder{xy};
	for (int i = 0; i < NCELLS; ++i) {
		int16_t* c = &cand[(size_t)i * 12];
		const int rr = finder.right(i), ll = finder.left(i), dd = finder.bottom(i), uu = finder.top(i);
		c[0] = (int16_t)rr; c[1] = (int16_t)ll; c[2] = (int16_t)dd; c[3] = (int16_t)uu;
		for (int k = 4; k < 12; ++k) c[k] = -1;
		if (rr >= 0 && ll >= 0) {
			const int h0 = finder.right(rr), h2 = finder.left(ll);
			c[4] = (int16_t)h0; c[5] = (int16_t)(h0 >= 0 ? finder.right(h0) : -1);
			c[6] = (int16_t)h2; c[7] = (int16_t)(h2 >= 0 ? finder.left(h2) : -1);
		}
		if (uu >= 0 && dd >= 0) {
			const int v0 = finder.top(uu), v2 = finder.bottom(dd);
			c[8] = (int16_t)v0; c[9] = (int16_t)(v0 >= 0 ? finder.top(v0) : -1);
			c[10] = (int16_t)v2; c[11] = (int16_t)(v2 >= 0 ? finder.bottom(v2) : -1);
		}
		// k_flood evaluates the twelve offers of a step independently: that needs them to be distinct cells
		for (int a = 0; a < 12; ++a)
			for (int b = a + 1; b < 12; ++b)
				if (c[a] >= 0 && c[a] == c[b]) { ctx->err = "build_tables: duplicate cell in a flood offer list"; return CIMBAR_HIP_EINVAL; }
	}
	// GF(2^8) tables, libcorrect field.h:26-62 with primitive polynomial 0x187 (correct.h:159-160)
	uint8_t gexp[512], glog[256];
	unsigned element = 1;
	gexp[0] = 1; glog[0] = 0;
	for (unsigned i = 1; i < 512; ++i) {
		element *= 2;
		if (element > 255) element ^= 0x187;
		gexp[i] = (uint8_t)element;
		if (i < 256) glog[element] = (uint8_t)i;
	}
	HIPCHK(ctx->tb_cell_xy.reserve(NCELLS));
	HIPCHK(ctx->tb_stream_cell.reserve(NCELLS));
	std::vector<uint16_t> cell_grid(NCELLS);
	for (int i = 0; i < NCELLS; ++i) cell_grid[i] = (uint16_t)((((int)xy[i].y - OFFSET) / PITCH) * DIM_X + ((int)xy[i].x - OFFSET) / PITCH);
	HIPCHK(ctx->tb_cell_grid.reserve(NCELLS));
	HIPCHK(hipMemcpy(ctx->tb_cell_grid, cell_grid.data(), sizeof(uint16_t) * NCELLS, hipMemcpyHostToDevice));
	std::vector<int16_t> grid_cell((size_t)DIM_X * DIM_Y, (int16_t)-1);
	for (int i = 0; i < NCELLS; ++i) grid_cell[cell_grid[i]] = (int16_t)i;
	HIPCHK(ctx->tb_grid_cell.reserve(grid_cell.size()));
	HIPCHK(hipMemcpy(ctx->tb_grid_cell, grid_cell.data(), sizeof(int16_t) * grid_cell.size(), hipMemcpyHostToDevice));
	std::vector<uint16_t> ccm_grid(NHDR_CELLS);
	for (int q = 0; q < NHDR_CELLS; ++q) {
		// CimbReader.cpp:188-196: header c starts at stream cell c * capacity(6 bits) * 8 / CHUNKS / 2 bits = c * NCELLS * 3 / CHUNKS
		const int cell = sc[(NCELLS / NHDR) * (q / 24) + q % 24];
		ccm_grid[q] = (uint16_t)((((int)xy[cell].y - OFFSET) / PITCH) * DIM_X + ((int)xy[cell].x - OFFSET) / PITCH);
	}
	HIPCHK(ctx->tb_ccm_grid.reserve(NHDR_CELLS));
	HIPCHK(hipMemcpy(ctx->tb_ccm_grid, ccm_grid.data(), sizeof(uint16_t) * NHDR_CELLS, hipMemcpyHostToDevice));
	std::vector<uint8_t> stitch_line((size_t)2 * NCELLS);
	for (int i = 0; i < NCELLS; ++i) {
		stitch_line[i] = (uint8_t)(((int)xy[i].y - OFFSET) / PITCH);
		stitch_line[NCELLS + i] = (uint8_t)(((int)xy[i].x - OFFSET) / PITCH);
	}
	HIPCHK(ctx->tb_stitch_line.reserve(stitch_line.size()));
	HIPCHK(hipMemcpy(ctx->tb_stitch_line, stitch_line.data(), stitch_line.size(), hipMemcpyHostToDevice));
	// the strips of cimbar_hip_set_stitch_strips: every line has cells in every strip, or a strip's flags would be empty products
	std::vector<uint16_t> stitch_width((size_t)2 * STITCH_SMAX * STITCH_SMAX * 128, 0);
	for (int axis = 0; axis < 2; ++axis)
		for (int S = 1; S <= STITCH_SMAX; ++S) {
			uint16_t* wt = stitch_width.data() + (size_t)(axis * STITCH_SMAX + S - 1) * STITCH_SMAX * 128;
			const int A = axis == 0 ? DIM_X : DIM_Y;
			for (int i = 0; i < NCELLS; ++i) ++wt[(stitch_line[(size_t)(axis ^ 1) * NCELLS + i] * S / A) * 128 + stitch_line[(size_t)axis * NCELLS + i]];
			for (int j = 0; j < S; ++j)
				for (int l = 0; l < stitch_lines(axis); ++l)
					if (!wt[j * 128 + l]) { ctx->err = "build_tables: a stitch strip without cells on a line"; return CIMBAR_HIP_EINVAL; }
		}
	HIPCHK(ctx->tb_stitch_width.reserve(stitch_width.size()));
	HIPCHK(hipMemcpy(ctx->tb_stitch_width, stitch_width.data(), sizeof(uint16_t) * stitch_width.size(), hipMemcpyHostToDevice));
	HIPCHK(ctx->tb_cand.reserve((size_t)NCELLS * 12));
	HIPCHK(hipMemcpy(ctx->tb_cell_xy, xy.data(), sizeof(ushort2) * NCELLS, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(ctx->tb_stream_cell, sc.data(), sizeof(uint16_t) * NCELLS, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(ctx->tb_cand, cand.data(), sizeof(int16_t) * NCELLS * 12, hipMemcpyHostToDevice));
	ctx->tb = Tables{ctx->tb_cell_xy, ctx->tb_stream_cell, ctx->tb_cell_grid, ctx->tb_grid_cell, ctx->tb_ccm_grid, ctx->tb_cand};
	HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_gf_exp), gexp, 512));
	HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_gf_log), glog, 256));
	// generator polynomial prod_{i=1..ecc_bytes} (x + alpha^i), low -> high (libcorrect reed-solomon.c:5-12, polynomial.c:205-240)
	uint8_t gen[RS_PARITY + 1] = {1};
	auto gmul = [&](uint8_t a, uint8_t b) -> uint8_t { return (!a || !b) ? 0 : gexp[(unsigned)glog[a] + glog[b]]; };
	for (int i = 0; i < RS_PARITY; ++i) {
		const uint8_t root = gexp[(i + 1) % 255];
		for (int j = i + 1; j >= 1; --j) gen[j] = gen[j - 1] ^ gmul(gen[j], root);
		gen[0] = gmul(gen[0], root);
	}
	uint8_t gen_log[RS_PARITY];
	for (int j = 0; j < RS_PARITY; ++j) gen_log[j] = glog[gen[j]];
	HIPCHK(ctx->d_gen_log.reserve(RS_PARITY));
	HIPCHK(hipMemcpy(ctx->d_gen_log, gen_log, RS_PARITY, hipMemcpyHostToDevice));
	return 0;
}

// the colour retry's margin buffer follows its scratch set: as many frames as the set holds, grown where the setting is on
int ensure_margin_capacity(cimbar_hip_ctx* ctx, cimbar_hip_ctx::ScratchSet& cur)
{
	if (ctx->ec_margin <= 0 || cur.cm_cap >= cur.cap) return 0;
	cur.cm_cap = 0;
	HIPCHK(cur.d_cmargin.reserve((size_t)cur.cap * (NCELLS + 1)));
	cur.cm_cap = cur.cap;
	return 0;
}

// room for a batch of n frames in the scratch set in use and in what every set shares
int ensure_capacity(cimbar_hip_ctx* ctx, int n)
{
	cimbar_hip_ctx::ScratchSet& cur = ctx->cur();
	size_t N = (size_t)n;
	// not part of the scratch sets: every set's batches stage their host-bound results here
	HIPCHK(ctx->d_chunks.reserve(N * FRAME_BYTES));
	HIPCHK(ctx->d_masks.reserve(N));
	HIPCHK(ctx->d_fw_queue.ensure((size_t)FW_GRID * NCELLS));
	if (n <= cur.cap) return ensure_margin_capacity(ctx, cur);
	cur.cap = 0;   // (what `d_flood + cap` and the taps read: never more than every buffer below holds)
	HIPCHK(cur.d_plane.reserve(N * PLANE_WORDS));
	HIPCHK(cur.d_cellmean.reserve(N * GRID_CELLS));
	HIPCHK(cur.d_symbols.reserve(N * NCELLS));
	HIPCHK(cur.d_colors.reserve(N * NCELLS));
	HIPCHK(cur.d_drift.reserve(N * NCELLS * 2));
	HIPCHK(cur.d_flood.reserve(3 * N));
	HIPCHK(hipMemset(cur.d_flood, 0, sizeof(uint32_t) * 3 * N));
	HIPCHK(cur.d_rs_ok.reserve(N * ALL_BLOCKS));
	HIPCHK(cur.d_states.reserve(N));
	HIPCHK(cur.d_ccm_frames.reserve(N * 10));
	HIPCHK(cur.d_ccm_used.reserve(N * 10));
	cur.cap = n;
	return ensure_margin_capacity(ctx, cur);
}

int ensure_verify_capacity(cimbar_hip_ctx* ctx, int n)
{
	if (n <= ctx->vcap) return 0;
	ctx->vcap = 0;
	HIPCHK(ctx->d_vsym.reserve((size_t)n * NCELLS));
	HIPCHK(ctx->d_vdrift.reserve((size_t)n * NCELLS * 2));
	HIPCHK(ctx->d_vflag.reserve((size_t)n * 2));
	HIPCHK(hipMemset(ctx->d_vflag, 0xFF, sizeof(uint32_t) * (size_t)n * 2));
	if (!ctx->d_vtotals) { HIPCHK(ctx->d_vtotals.reserve(2)); HIPCHK(hipMemset(ctx->d_vtotals, 0, 2 * sizeof(unsigned long long))); }
	ctx->vcap = n;
	return 0;
}

// host-resident input of a call goes through a device buffer of the context (grown on demand): *d = where the kernels read it
int stage_input(cimbar_hip_ctx* ctx, hipStream_t st, DevBuf<uint8_t>& buf, const uint8_t* src, size_t bytes, int mem, const uint8_t** d)
{
	*d = src;
	if (mem == CIMBAR_HIP_MEM_HOST) {
		HIPCHK(buf.reserve(bytes));
		HIPCHK(hipMemcpyAsync(buf, src, bytes, hipMemcpyHostToDevice, st));
		*d = buf;
	}
	return 0;
}

// ... and host-bound output: *d = where the kernels write it (the caller copies it back)
int stage_output(cimbar_hip_ctx* ctx, DevBuf<uint8_t>& buf, uint8_t* dst, size_t bytes, int mem, uint8_t** d)
{
	*d = dst;
	if (mem == CIMBAR_HIP_MEM_HOST) {
		HIPCHK(buf.reserve(bytes));
		*d = buf;
	}
	return 0;
}

// pipelined batches in flight use the scratch sets and the tail stream: anything else that touches them on `st` waits first
int drain_pipeline_into(cimbar_hip_ctx* ctx, hipStream_t st)
{
	for (int k = 0; k < cimbar_hip_ctx::MAXP; ++k)
		if (ctx->pipe_used[k]) HIPCHK(hipStreamWaitEvent(st, ctx->ev_pdone[k], 0));   // (a completed event costs nothing to wait for)
	return 0;
}

// a call's mem flags, named in the message as the entry point's own arguments are (in_name == nullptr: the call has the one flag, out_name's)
int check_mem_flags(cimbar_hip_ctx* ctx, const char* who, const char* in_name, int in_mem, const char* out_name, int out_mem)
{
	if ((!in_name || in_mem == CIMBAR_HIP_MEM_HOST || in_mem == CIMBAR_HIP_MEM_DEVICE) && (out_mem == CIMBAR_HIP_MEM_HOST || out_mem == CIMBAR_HIP_MEM_DEVICE)) return 0;
	ctx->err = std::string(who) + ": " + (in_name ? std::string(in_name) + " / " : std::string()) + out_name + " must be CIMBAR_HIP_MEM_HOST or CIMBAR_HIP_MEM_DEVICE";
	return CIMBAR_HIP_EINVAL;
}

// The prologue of every batch call, behind its own null / n checks: the mem flags, the device, the stream the call runs on (*st) and the
// wait for the pipelined batches in flight. A NULL hip_stream means what it means for any HIP launch -- the (legacy) null stream -- whenever
// a device buffer is involved, so the work is ordered after whatever produced the input there; the all-host path synchronises anyway and
// uses the context's own stream.
int begin_call(cimbar_hip_ctx* ctx, const char* who, const char* in_name, int in_mem, const char* out_name, int out_mem, void* hip_stream, hipStream_t* st)
{
	if (int r = check_mem_flags(ctx, who, in_name, in_mem, out_name, out_mem)) return r;
	HIPCHK(hipSetDevice(ctx->device));
	const bool any_device = (in_name && in_mem == CIMBAR_HIP_MEM_DEVICE) || out_mem == CIMBAR_HIP_MEM_DEVICE;
	*st = hip_stream ? (hipStream_t)hip_stream : (any_device ? (hipStream_t)nullptr : ctx->stream);
	return drain_pipeline_into(ctx, *st);
}

// the next batch (or frame) takes the next set
void rotate_scratch_sets(cimbar_hip_ctx* ctx) { ctx->pipe_set = (ctx->pipe_set + 1) % ctx->pipe_depth; }

// one spill area (HEAP_CAP words, and PRIO_STRIDE bytes for the dense instance: 0.61 MB) per flood workgroup a launch may start, [0, count): grown on
// demand -- a context that only ever decodes single frames through the plain calls keeps 0.6 MB (through the pipelined ones, whose last set starts at
// 2 (depth - 1) areas: 830 MB at depth 3), not the 620 MB .. 1.25 GB a 1024-frame batch wants. Growing replaces the buffer, so everything in flight is
// waited for first. `count` is ChainPlan::flood_top. Its one spacing for every instance (chainplan.hip.inc) costs device memory where the batches stay
// small: a pipelined set's batch of n <= areas frames asks for 2 (depth - 1) areas + n, not (depth - 1) areas + n (depth 3: 682 areas = 415 MB more), a
// split batch of up to 512 frames for 1024 + n, not 512 + n (310 MB more); larger batches were sized in these units already.
int ensure_flood_areas(cimbar_hip_ctx* ctx, int count)
{
	if (count <= ctx->flood_cap) return 0;
	HIPCHK(hipDeviceSynchronize());
	ctx->flood_cap = 0;
	HIPCHK(ctx->flood_heap.reserve((size_t)count * HEAP_CAP));
	HIPCHK(ctx->flood_prio.reserve((size_t)count * PRIO_STRIDE));
	if (!ctx->flood_next) { HIPCHK(ctx->flood_next.reserve((size_t)2 * FLOOD_COUNTERS)); HIPCHK(hipMemset(ctx->flood_next, 0, sizeof(uint32_t) * 2 * FLOOD_COUNTERS)); }
	ctx->flood = FloodScratch{ctx->flood_heap, ctx->flood_next, ctx->flood_prio};
	ctx->flood_cap = count;
	return 0;
}

constexpr int K1_TALL_MIN = 256;   // frames: 16 tall strips x 256 = 4 096 wavefronts, more than the 3 072 the chip holds
// erasures per retried block: the setting, or the default RS_PARITY - 8 (at most 4 errors beside them; DESIGN_WIDENING.md "Erasure decoding":
// with 2 the decoder accepts a wrong codeword for about one garbage block in eight)
constexpr int ERASURE_MAX_DEFAULT = RS_PARITY - 8;
inline int erasure_max(const cimbar_hip_ctx* ctx) { return ctx->er_max < 0 ? ERASURE_MAX_DEFAULT : ctx->er_max; }
inline int colour_erasure_max(const cimbar_hip_ctx* ctx) { return ctx->ec_max < 0 ? ERASURE_MAX_DEFAULT : ctx->ec_max; }

// an image larger than the frame (CimbReader's _gridPadding case, decode_frame): K1p cuts the grid's window out of it while it thresholds it
struct PadSource { const uint8_t* pad_src = nullptr; int pad_w = 0, pad_h = 0, pad_off = 0; };

// One batch as enqueue() takes it. What the chain for it looks like -- one chain, a pipelined set's, or parts on two streams; each lane's spill
// areas, wave queues and counter; the exact replay's instance and grid -- is not decided here or in enqueue(): plan_chain() in chainplan.hip.inc
// states that rule once, from these arguments and the context's settings, and tests/test_chain_plan.py checks it without a GPU.
struct ChainArgs {
	const uint8_t* d_rgb = nullptr; int n = 0;      // n device-resident frames
	int pre = 0, cc = 0;                            // sharpen every frame; the colour-correction setting
	uint8_t* d_chunks = nullptr; uint32_t* d_masks = nullptr;   // device-visible outputs
	int plain = 0;                                  // the plain stream (decode_plain_batch)
	bool pipe = false;                              // one set of the pipeline: the whole chain on `st`, the carry from the set before
	const int* d_sel = nullptr; int sel_stride = 0; // not null: sharpen where the extractor's verdict says so, per frame (`pre` is then not read)
	bool symbols_only = false;                      // stop behind k_frame_mid (auto_symbols: the colour half is issued later)
	bool no_split = false;                          // one chain, never two half-batches: deskewed captures all take the exact flood, and two half-batch flood
	                                                // launches on two queues run one after the other in effect (1024 captures: 62 ms split, 42 ms as one launch)
	PadSource pad{};                                // n == 1 only; d_rgb is then where K1p leaves the window
};

// What the stages of one enqueue() share. The plan (chainplan.hip.inc) says what to launch; the stages below issue it and decide nothing.
struct Chain {
	cimbar_hip_ctx* ctx; cimbar_hip_ctx::ScratchSet& cur; const ChainArgs& a; const ChainPlan& plan;
	hipStream_t st;        // the caller's stream (or the pipelined set's)
	bool timed;            // stage timing: only ever a single chain on `st` (a timed batch is neither pipelined nor split)
	bool relaxed;          // the relaxed flood (cimbar_hip_set_relaxed_flood) is on
	bool colour_retry;     // the colour retry (erasure.hip.inc) runs behind every chain that reports chunks; the set in use holds its margins
};
static_assert(cimbar_hip_ctx::MAXP <= FLOOD_COUNTERS && 2 <= FLOOD_COUNTERS, "a counter pair per pipelined set and per stream of a split batch");

// stage boundary k of a timed batch (STAGE_NAMES[k] lies between k and k + 1)
inline hipError_t mark(const Chain& c, int k) { return c.timed ? hipEventRecord(c.ctx->ev[k], c.st) : hipSuccess; }

template <int RAD, bool PRE, bool TALL>
void launch_k1(const Chain& c, const int* d_sel, int sel_stride, int lds)
{
	hipLaunchKernelGGL((k_threshold<RAD, PRE, TALL ? K1_TALLROWS : K1_CELLROWS>), dim3(TALL ? K1_TALL_BLOCKS : K1_BLOCKS, c.a.n), dim3(256), (size_t)lds, c.st,
	                   c.a.d_rgb, c.cur.d_plane, c.cur.d_cellmean, c.cur.d_flood, 0, d_sel, sel_stride);
}

// K1 for the whole batch, on the caller's stream
void launch_threshold(const Chain& c)
{
	const cimbar_hip_ctx* ctx = c.ctx; const ChainArgs& a = c.a; cimbar_hip_ctx::ScratchSet& cur = c.cur;
	if (a.pad.pad_src && a.n == 1) {
		// the frame buffer d_rgb is OUTPUT here: K1p cuts the grid's window out of the larger image while it thresholds it
		uint8_t* frame = const_cast<uint8_t*>(a.d_rgb);
		const dim3 gp((IMG_W + 63) / 64, (IMG_H + 3) / 4);
		const PadSource& p = a.pad;
		if (a.pre) hipLaunchKernelGGL((k_threshold_padded<3, true>), gp, dim3(256), 0, c.st, p.pad_src, p.pad_w, p.pad_h, p.pad_off, cur.d_plane, frame, cur.d_flood);
		else hipLaunchKernelGGL((k_threshold_padded<2, false>), gp, dim3(256), 0, c.st, p.pad_src, p.pad_w, p.pad_h, p.pad_off, cur.d_plane, frame, cur.d_flood);
		hipLaunchKernelGGL(k_cellmean_padded, dim3((GRID_CELLS + 255) / 256), dim3(256), 0, c.st, frame, cur.d_cellmean);
		return;
	}
	// the sharpening variant is bound by its vector instructions (96 % of its cycles), not by the memory system: tall strips (69 row steps for 63
	// rows instead of 24 for 18) shorten the launch itself, pipelined or not, once the batch fills the chip with them; the plain one takes them
	// inside the pipelined loop (fewer row steps and halo rows per frame; the uneven drain is covered by the other batches in flight)
	const bool tall = ctx->k1_tall > 0 || (ctx->k1_tall < 0 && a.n >= K1_TALL_MIN);
	const bool sharp_tall = tall, plain_tall = tall && (ctx->k1_tall > 0 || a.pipe);
	// pre == -1 ("guess", cimbar.cpp:190): the extractor's verdict decides per frame; each variant returns at once for the other's frames.
	// CIMBAR_HIP_K1_LDS_PAD caps the occupancy of the plain variant where it runs alone.
	const int* sel = a.d_sel; const int stride = sel ? a.sel_stride : 0;
	if (sel || a.pre) { if (sharp_tall) launch_k1<3, true, true>(c, sel, stride, 0); else launch_k1<3, true, false>(c, sel, stride, 0); }
	if (sel) launch_k1<2, false, false>(c, sel, stride, 0);
	else if (!a.pre) { if (plain_tall) launch_k1<2, false, true>(c, nullptr, 0, ctx->k1_lds_pad); else launch_k1<2, false, false>(c, nullptr, 0, ctx->k1_lds_pad); }
}

// One exact replay (k_flood3) of a part's frames flagged in `flags`: the instance and grid are the plan's, the spill areas and the counter pair
// its lane's. kind: CIMBAR_HIP_TAP_FLOOD_LAUNCH's flags (0 the batch's own, 1 the verify replay, 2 the relaxed flood's fallback).
void launch_exact_flood(const Chain& c, hipStream_t s, const ChainPart& p, const uint32_t* flags, int kind)
{
	cimbar_hip_ctx* ctx = c.ctx; cimbar_hip_ctx::ScratchSet& cur = c.cur;
	if (ctx->dbg_skip & 2) return;
	const ChainLane& L = c.plan.lane[p.lane];
	const ExactLaunch x = exact_launch(c.plan, p.lane, p.count);
	if (ctx->flood_launch_n < FLOOD_LAUNCH_MAX) {
		const int32_t rec[7] = {x.instance, x.grid, p.count, p.first, L.area0, L.counter, kind};
		std::memcpy(ctx->flood_launch[ctx->flood_launch_n++], rec, sizeof rec);
	}
	// a launch with fewer workgroups than frames hands the rest out through the counter pair sc.next[2 * counter ..]: zeroed HERE, in stream
	// order in front of the launch, so that a launch that faulted or was aborted cannot leave the pair non-zero for the ones after it
	if (x.hand_out) (void)hipMemsetAsync(ctx->flood.next + 2 * L.counter, 0, 2 * sizeof(uint32_t), s);
	const dim3 grid(x.grid);
	if (x.instance == 8) hipLaunchKernelGGL((k_flood3<HEAP_LDS8, true>), grid, dim3(128), 0, s, cur.d_plane, ctx->tb, ctx->flood, flags, cur.d_symbols, cur.d_drift, p.first, p.count, L.area0, L.counter);
	else if (x.instance == 3) hipLaunchKernelGGL((k_flood3<HEAP_LDS, false>), grid, dim3(128), 0, s, cur.d_plane, ctx->tb, ctx->flood, flags, cur.d_symbols, cur.d_drift, p.first, p.count, L.area0, L.counter);
	else hipLaunchKernelGGL((k_flood3<HEAP_LDS4, false>), grid, dim3(128), 0, s, cur.d_plane, ctx->tb, ctx->flood, flags, cur.d_symbols, cur.d_drift, p.first, p.count, L.area0, L.counter);
}

// The front half of the chain for one part, on stream s: symbols -> flood -> RS -> k_frame_mid (header / CCM)
hipError_t chain_front(const Chain& c, hipStream_t s, const ChainPart& p)
{
	cimbar_hip_ctx* ctx = c.ctx; cimbar_hip_ctx::ScratchSet& cur = c.cur; const ChainArgs& a = c.a;
	const ChainLane& L = c.plan.lane[p.lane];
	const int fa = p.first, m = p.count;
	if (!(ctx->dbg_skip & 1)) hipLaunchKernelGGL(k_symbols, dim3(K2_BLOCKS, m), dim3(256), 0, s, cur.d_plane, ctx->tb, cur.d_symbols, cur.d_flood, fa);
	if (hipError_t e = mark(c, 2)) return e;
	if (c.plan.run_wave && !(ctx->dbg_skip & 2)) {
		// first the batch-parallel pass for frames whose flood provably does not depend on the tie order (it clears their flag to 2)
		hipLaunchKernelGGL(k_flood_wave, dim3(m < L.wareas ? m : L.wareas), dim3(256), 0, s, cur.d_plane, ctx->tb, ctx->d_fw_queue, cur.d_flood,
		                   cur.d_symbols, cur.d_drift, fa, m, L.warea0, cur.d_flood + cur.cap);
	} else if (ctx->flood_wave && !(ctx->dbg_skip & 2)) {
		// skipped by the scheduler: CIMBAR_HIP_TAP_FLOOD_INFO must not show what the pass said about some earlier batch
		if (hipError_t e = hipMemsetAsync(cur.d_flood + cur.cap + fa, 0xFF, sizeof(uint32_t) * (size_t)m, s)) return e;
	}
	// The relaxed flood (cimbar_hip_set_relaxed_flood): the frames still flagged 1 are flooded in threshold rounds (flag 3) instead of
	// replayed; what the symbol streams' RS pass makes of them decides below whether they stay that way.
	if (c.relaxed) {
		if (hipError_t e = hipMemsetAsync(cur.d_flood + 2 * cur.cap + fa, 0, sizeof(uint32_t) * (size_t)m, s)) return e;
		hipLaunchKernelGGL(k_flood_rounds, dim3(m < ctx->rf_grid ? m : ctx->rf_grid), dim3(FR_THREADS), 0, s, cur.d_plane, ctx->tb, cur.d_flood, cur.d_symbols,
		                   cur.d_drift, fa, m, (uint32_t)ctx->rf_threshold, cur.d_flood + 2 * cur.cap);
	}
	if (c.plan.exact_batch) launch_exact_flood(c, s, p, cur.d_flood, 0);
	if (c.plan.exact_verify && !(ctx->dbg_skip & 2)) {
		// CIMBAR_HIP_FLOOD_VERIFY: what k_flood_wave certified (flag 2) is set aside, the same frames are replayed exactly, and the two
		// results are compared cell by cell (symbol and drifted position). The exact result is what stays -- a wrong certificate would be
		// counted (cimbar_hip_flood_verify_totals, CIMBAR_HIP_TAP_FLOOD_VERIFY) AND repaired.
		hipLaunchKernelGGL(k_verify_begin, dim3(m), dim3(256), 0, s, cur.d_flood, cur.d_symbols, cur.d_drift, ctx->d_vflag, ctx->d_vsym, ctx->d_vdrift, fa, ctx->vcap);
		launch_exact_flood(c, s, p, ctx->d_vflag, 1);
		hipLaunchKernelGGL(k_verify_end, dim3(m), dim3(256), 0, s, cur.d_symbols, cur.d_drift, ctx->d_vflag, ctx->d_vsym, ctx->d_vdrift, fa, ctx->vcap, ctx->d_vtotals);
	}
	if (hipError_t e = mark(c, 3)) return e;
	// (legacy modes have ONE stream, decoded after the colour pass; the stage-time slot stays so that the names keep their meaning)
#ifdef CIMBAR_PROBES
	if (!LEGACY && (ctx->dbg_skip & 128)) hipLaunchKernelGGL((k_rs<4, true>), dim3((m * SYM_BLOCKS + 3) / 4), dim3(256), 0, s, cur.d_symbols, ctx->tb, fa, m, 0, a.d_chunks, cur.d_rs_ok, 0, (const uint8_t*)nullptr);
	else
#endif
	if (!LEGACY && !(ctx->dbg_skip & 4)) hipLaunchKernelGGL((k_rs<4>), dim3((m * SYM_BLOCKS + 3) / 4), dim3(256), 0, s, cur.d_symbols, ctx->tb, fa, m, 0, a.d_chunks, cur.d_rs_ok, 0);
	if (c.relaxed) {
		// acceptance: a frame flooded in rounds keeps its result iff every symbol block decoded. With fallback on, the others go back to flag 1,
		// the exact replay takes them -- inside this call, in front of everything that reads symbols, drift or flags -- and the RS pass runs once
		// more over the part (it rewrites the same bytes for the frames that did not change: 40 blocks per frame of clean-path work).
		hipLaunchKernelGGL(k_rounds_check, dim3((m + 255) / 256), dim3(256), 0, s, cur.d_flood, cur.d_rs_ok, cur.d_flood + 2 * cur.cap, fa, m, ctx->rf_fallback, ctx->d_rf_stats);
		if (c.plan.exact_fallback) {
			launch_exact_flood(c, s, p, cur.d_flood, 2);
			hipLaunchKernelGGL((k_rs<4>), dim3((m * SYM_BLOCKS + 3) / 4), dim3(256), 0, s, cur.d_symbols, ctx->tb, fa, m, 0, a.d_chunks, cur.d_rs_ok, 0);
		}
	}
	if (hipError_t e = mark(c, 4)) return e;
	if (!(ctx->dbg_skip & 8)) hipLaunchKernelGGL(k_frame_mid, dim3(m), dim3(64), 0, s, a.d_rgb, cur.d_cellmean, ctx->tb, a.d_chunks, cur.d_rs_ok, a.cc, cur.d_states, cur.d_ccm_frames, fa, a.plain);
	return mark(c, 5);
}

// The back half for one part, on stream s: colours -> RS -> k_frame_end (masks, carry), then the erasure retries
hipError_t chain_back(const Chain& c, hipStream_t s, const ChainPart& p)
{
	cimbar_hip_ctx* ctx = c.ctx; cimbar_hip_ctx::ScratchSet& cur = c.cur; const ChainArgs& a = c.a;
	const int fa = p.first, m = p.count;
	if (!(ctx->dbg_skip & 16)) hipLaunchKernelGGL((k_colors<false>), dim3(K5_BLOCKS, m), dim3(256), 0, s, a.d_rgb, cur.d_cellmean, ctx->tb, cur.d_ccm_frames,
	                   ctx->d_carry, cur.d_flood, cur.d_drift, cur.d_colors, cur.d_ccm_used, fa);
	if (hipError_t e = mark(c, 6)) return e;
	if (LEGACY) hipLaunchKernelGGL((k_rs<(LEGACY ? CELL_BITS : 6)>), dim3((m * ALL_BLOCKS + 3) / 4), dim3(256), 0, s, cur.d_symbols, ctx->tb, fa, m, 0, a.d_chunks, cur.d_rs_ok, 0, cur.d_colors);
#ifdef CIMBAR_PROBES
	else if (ctx->dbg_skip & 128) hipLaunchKernelGGL((k_rs<2, true>), dim3((m * COL_BLOCKS + 3) / 4), dim3(256), 0, s, cur.d_colors, ctx->tb, fa, m, SYM_CHUNKS, a.d_chunks, cur.d_rs_ok, SYM_BLOCKS, (const uint8_t*)nullptr);
#endif
	else if (!(ctx->dbg_skip & 32)) hipLaunchKernelGGL((k_rs<2>), dim3((m * COL_BLOCKS + 3) / 4), dim3(256), 0, s, cur.d_colors, ctx->tb, fa, m, SYM_CHUNKS, a.d_chunks, cur.d_rs_ok, SYM_BLOCKS);
	if (hipError_t e = mark(c, 7)) return e;
	// (split chain: the carry is written by k_carry_out after the join -- an earlier part's colour pass may still be reading the old one)
	if (!(ctx->dbg_skip & 64)) hipLaunchKernelGGL(k_frame_end, dim3(m), dim3(64), 0, s, cur.d_rs_ok, cur.d_states, a.d_chunks, a.d_masks, cur.d_ccm_used, ctx->d_carry, fa,
	                   (!c.plan.split && fa + m == a.n) ? 1 : 0, a.plain);
	// opt-in erasure retry of the symbol chunks the mask lacks (erasure.hip.inc); reads the frame's own intermediates only, writes its
	// chunks and mask: the same stream, after k_frame_end, in every chain shape (split halves, pipelined sets)
	if (!LEGACY && !a.plain && ctx->er_sym > 0)
		hipLaunchKernelGGL(k_erasure_frame, dim3(m), dim3(256), 0, s, cur.d_plane, ctx->tb, cur.d_symbols, cur.d_drift, cur.d_flood, cur.d_rs_ok,
		                   a.d_chunks, a.d_masks, fa, ctx->er_sym, erasure_max(ctx));
	// ... and of the colour chunks it lacks (cimbar_hip_set_colour_erasure_decode), independent of the symbol retry and behind it
	if (c.colour_retry)
		hipLaunchKernelGGL(k_colour_erasure_frame, dim3(m), dim3(256), 0, s, a.d_rgb, cur.d_cellmean, ctx->tb, cur.d_colors, cur.d_drift, cur.d_flood,
		                   cur.d_ccm_used, cur.d_rs_ok, a.d_chunks, a.d_masks, cur.d_cmargin, cur.d_cmargin + (size_t)cur.cm_cap * NCELLS, fa,
		                   ctx->ec_margin, colour_erasure_max(ctx));
	return mark(c, 8);
}

// Enqueue the whole chain for a.n device-resident frames on stream `st`: plan it (plan_chain, from one snapshot of the context's settings and
// of what the batch before reported), make room, note what the taps will be asked about, launch K1, then drive the parts of the plan.
// Everything after K1 is a chain of small kernels per frame (symbols -> flood -> RS -> header/CCM -> colours -> RS -> masks), some of
// them latency-bound (k_frame_mid is one serial wavefront per frame). For a large batch the chain runs as parts on two streams, so one
// part's serial phases and launch gaps are covered by the other's kernels. The only cross-part dependency is the colour-correction carry:
// a frame with no matrix of its own takes the newest one of the frames before it, so a part's colour pass waits for k_frame_mid of the
// part before. Stage timing uses the single-stream order.
int enqueue(cimbar_hip_ctx* ctx, hipStream_t st, const ChainArgs& a)
{
	const int n = a.n;
	cimbar_hip_ctx::ScratchSet& cur = ctx->cur();
	const bool colour_retry = !LEGACY && !a.plain && !a.symbols_only && ctx->ec_margin > 0;
	if (colour_retry) { if (int r = ensure_margin_capacity(ctx, cur)) return r; }
	const bool relaxed = !LEGACY && ctx->rf_threshold >= 0 && ctx->d_rf_stats && !(ctx->dbg_skip & 2);

	ChainPlanIn in;
	in.n = n; in.pipe = a.pipe; in.no_split = a.no_split; in.symbols_only = a.symbols_only;
	in.timed = ctx->timing && !a.pipe;
	// What the batch before reported (k_count_flagged writes these pinned words asynchronously -- a device-output call returns without a
	// sync -- so they are read ONCE here; a stale value only costs the heuristic).
	in.have_flagged = ctx->h_flagged != nullptr;
	if (in.have_flagged) for (int k = 0; k < 3; ++k) in.flagged[k] = ((volatile uint32_t*)ctx->h_flagged)[k];
	in.tail_split = ctx->tail_split; in.tail_parts = ctx->tail_parts; in.pipe_depth = ctx->pipe_depth; in.pipe_set = ctx->pipe_set;
	in.flood_dense = ctx->flood_dense; in.flood_dense_grid = ctx->flood_dense_grid;
	in.flood_wave = ctx->flood_wave; in.flood_verify = ctx->flood_verify; in.wave_adapt = ctx->wave_adapt;
	in.wave_ran = ctx->wave_ran; in.wave_skip_left = ctx->wave_skip_left;
	in.relaxed = relaxed; in.relaxed_fallback = ctx->rf_fallback != 0;
	const ChainPlan plan = plan_chain(in);

	if (int r = ensure_flood_areas(ctx, plan.flood_top)) return r;
	if (ctx->flood_verify) if (int r = ensure_verify_capacity(ctx, n)) return r;

	// the context's bookkeeping of this batch (a call that could not make room has left the last batch's in place)
	ctx->grp_valid = false;   // (the group taps describe a combined batch only until the next batch of any kind)
	ctx->stitch_n = 0;        // (... and the stitch taps a stitched one)
	ctx->gcv_valid = false;
	ctx->gcv_stream_n = -1;
	ctx->cm_valid = colour_retry;
	ctx->rf_valid = relaxed;
	ctx->flood_launch_n = 0;  // (launch_exact_flood appends)
	ctx->flood_launch_top = plan.flood_top;
	ctx->wave_ran = plan.wave_ran;
	ctx->wave_skip_left = plan.wave_skip_left;
	ctx->last_n = n;

	const Chain c{ctx, cur, a, plan, st, in.timed, relaxed, colour_retry};
	HIPCHK(mark(c, 0));
	launch_threshold(c);
	HIPCHK(mark(c, 1));
	const ChainPart* const part = plan.part;
	if (a.pipe) {
		// the whole batch runs on one of the context's pipeline streams (`st` here), the next batch on the next one: independent
		// queues, so K1 of one batch overlaps the short kernels of the others. The one thing that crosses over is the colour-
		// correction carry (and the order of the results): this batch's colour pass waits for the previous batch's end.
		const int set = ctx->pipe_set, prev = (set + ctx->pipe_depth - 1) % ctx->pipe_depth;
		HIPCHK(chain_front(c, st, part[0]));
		if (ctx->pipe_used[prev]) HIPCHK(hipStreamWaitEvent(st, ctx->ev_pdone[prev], 0));
		HIPCHK(chain_back(c, st, part[0]));
		HIPCHK(hipEventRecord(ctx->ev_pdone[set], st));
		ctx->pipe_used[set] = true;
		ctx->pipe_gathered[set] = false;
	} else if (!plan.split) {
		HIPCHK(chain_front(c, st, part[0]));
		// (symbols_only: the mode auto-detection runs the colour half itself, once the matrix in force is known per frame: automode_mode.hip.inc)
		if (!plan.stop_at_mid) HIPCHK(chain_back(c, st, part[0]));
	} else {
		// lane 0 is the caller's stream, lane 1 stream2; pairs of parts are issued together so that both streams always have work
		const hipStream_t lane[2] = {st, ctx->stream2};
		HIPCHK(hipEventRecord(ctx->ev_k1, st));
		HIPCHK(hipStreamWaitEvent(lane[1], ctx->ev_k1, 0));
		for (int p = 0; p < plan.nparts; p += 2) {
			for (int q = p; q < p + 2; ++q) {
				HIPCHK(chain_front(c, lane[part[q].lane], part[q]));
				HIPCHK(hipEventRecord(ctx->ev_mid[q], lane[part[q].lane]));
			}
			for (int q = p; q < p + 2; ++q) {
				if (q > 0) HIPCHK(hipStreamWaitEvent(lane[part[q].lane], ctx->ev_mid[q - 1], 0));   // every k_frame_mid of the frames before this part is done
				HIPCHK(chain_back(c, lane[part[q].lane], part[q]));
			}
		}
		HIPCHK(hipEventRecord(ctx->ev_join, lane[1]));
		HIPCHK(hipStreamWaitEvent(st, ctx->ev_join, 0));
		hipLaunchKernelGGL(k_carry_out, dim3(1), dim3(64), 0, st, cur.d_ccm_used, ctx->d_carry, n - 1);
	}
	if (plan.counted) hipLaunchKernelGGL(k_count_flagged, dim3(1), dim3(256), 0, st, cur.d_flood, n, ctx->h_flagged);
	HIPCHK(hipGetLastError());
	return 0;
}

}  // namespace

// ---- the C ABI of this mode (same names as include/cimbar_hip.h; api.hip.inc holds the extern "C" entry points that dispatch here)

int cimbar_hip_bufsize(void) { return FRAME_BYTES; }
int cimbar_hip_ctx_bufsize(const cimbar_hip_ctx* ctx) { return ctx ? FRAME_BYTES : CIMBAR_HIP_EINVAL; }
static_assert(FRAME_BYTES <= CIMBAR_HIP_MAX_FRAME_BYTES, "include/cimbar_hip.h: CIMBAR_HIP_MAX_FRAME_BYTES must hold every mode's frame payload");

int cimbar_hip_tile_hashes(uint64_t out16[16])
{
	if (!out16) return CIMBAR_HIP_EINVAL;
	compute_tile_hashes(out16);
	return 16;
}

int cimbar_hip_geometry(const cimbar_hip_ctx* ctx, int32_t out[CIMBAR_HIP_GEOMETRY_WORDS])
{
	if (!ctx || !out) return CIMBAR_HIP_EINVAL;
	const int32_t g[CIMBAR_HIP_GEOMETRY_WORDS] = {MODE_VAL, IMG_W, IMG_H, NCELLS, CHUNKS, CHUNK, ALL_BLOCKS, RS_BLOCK, RS_PARITY, DIM_X, DIM_Y, OFFSET};
	std::memcpy(out, g, sizeof g);
	return CIMBAR_HIP_GEOMETRY_WORDS;
}

// what comm.hip.inc needs of a context
void ctx_view(cimbar_hip_ctx* ctx, int* device, std::string** err, int* frame_bytes) { *device = ctx->device; *err = &ctx->err; *frame_bytes = FRAME_BYTES; }
// what deliver.hip.inc needs of one
void delivery_view(cimbar_hip_ctx* ctx, deliver::View* v)
{
	v->device = ctx->device; v->err = &ctx->err; v->stream = ctx->stream; v->chunk = CHUNK; v->per = CHUNKS; v->state = &ctx->delivery;
}
// ... and of its pipeline: the stream the batch issued last through cimbar_hip_decode_batch_pipelined runs on, and the event that says "that batch is done"
// (false: no pipelined batch has been issued yet)
bool ctx_pipe_view(cimbar_hip_ctx* ctx, hipStream_t* stream, hipEvent_t* gathered)
{
	const int set = ctx->pipe_set;
	if (!ctx->pipe_used[set]) return false;
	*stream = ctx->pstream[set];
	*gathered = ctx->ev_pgather[set];
	ctx->pipe_gathered[set] = true;          // (the caller records the event behind its exchange)
	return true;
}

int cimbar_hip_create(int device, int mode_val, cimbar_hip_ctx** out)
{
	if (!out) return CIMBAR_HIP_EINVAL;
	*out = nullptr;
	if (mode_val != MODE_VAL) return CIMBAR_HIP_EINVAL;                // api.hip.inc picked this namespace by mode_val
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return CIMBAR_HIP_ENODEVICE;
	if (hipSetDevice(device) != hipSuccess) return CIMBAR_HIP_ENODEVICE;
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) != hipSuccess) return CIMBAR_HIP_ENODEVICE;
	if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return CIMBAR_HIP_ENODEVICE;   // kernels are built for gfx950 only

	cimbar_hip_ctx* ctx = new cimbar_hip_ctx();
	ctx->device = device;
	auto fail = [&](int code) { delete ctx; return code; };
	if (ctx->stream.create() != hipSuccess || ctx->stream2.create() != hipSuccess) return fail(CIMBAR_HIP_EHIP);
	if (const char* v = std::getenv("CIMBAR_HIP_PIPE_DEPTH")) { int k = std::atoi(v); if (k >= 2 && k <= cimbar_hip_ctx::MAXP) ctx->pipe_depth = k; }
	// As few streams as possible: the runtime multiplexes streams onto (by default) four hardware queues, and how the pipeline's
	// streams fall onto them matters (measured, 1024-frame batches: depth 4 over six streams 0.81 ms per batch, slower than depth 2;
	// depth 4 over these four streams 0.68 ms; raising GPU_MAX_HW_QUEUES to 8 made it worse again). So the pipeline reuses the two
	// streams the context has anyway and adds only what the depth needs beyond them.
	ctx->pstream[0] = ctx->stream;
	ctx->pstream[1] = ctx->stream2;
	for (int k = 2; k < ctx->pipe_depth; ++k) {
		if (ctx->pstream_own[k].create() != hipSuccess) return fail(CIMBAR_HIP_EHIP);
		ctx->pstream[k] = ctx->pstream_own[k];
	}
	for (Event* e : {&ctx->ev_k1, &ctx->ev_join})
		if (e->create() != hipSuccess) return fail(CIMBAR_HIP_EHIP);
	for (Event& e : ctx->ev_mid) if (e.create() != hipSuccess) return fail(CIMBAR_HIP_EHIP);
	for (Event& e : ctx->ev_pk1) if (e.create() != hipSuccess) return fail(CIMBAR_HIP_EHIP);
	for (Event& e : ctx->ev_pdone) if (e.create() != hipSuccess) return fail(CIMBAR_HIP_EHIP);
	for (Event& e : ctx->ev_pgather) if (e.create() != hipSuccess) return fail(CIMBAR_HIP_EHIP);
	if (const char* v = std::getenv("CIMBAR_HIP_TAIL_SPLIT")) ctx->tail_split = std::atoi(v);
	if (const char* v = std::getenv("CIMBAR_HIP_FLOOD_WAVE")) ctx->flood_wave = std::atoi(v) != 0;
	if (const char* v = std::getenv("CIMBAR_HIP_FLOOD_WAVE_ADAPT")) ctx->wave_adapt = std::atoi(v) != 0;
	if (const char* v = std::getenv("CIMBAR_HIP_FLOOD_VERIFY")) ctx->flood_verify = std::atoi(v) != 0;
	if (const char* v = std::getenv("CIMBAR_HIP_FLOOD_DENSE")) ctx->flood_dense = std::atoi(v);
	if (const char* v = std::getenv("CIMBAR_HIP_FLOOD_DENSE_GRID")) { int k = std::atoi(v); if (k >= 4 && k <= FLOOD_DENSE_PER * FLOOD_GRID) ctx->flood_dense_grid = k; }
	if (const char* v = std::getenv("CIMBAR_HIP_ROUNDS_GRID")) { int k = std::atoi(v); if (k >= 1 && k <= FR_GRID) ctx->rf_grid = k; }
#ifdef CIMBAR_PROBES
	if (const char* v = std::getenv("CIMBAR_HIP_DEBUG_SKIP")) ctx->dbg_skip = std::atoi(v);
#endif
	if (const char* v = std::getenv("CIMBAR_HIP_FRAME_STAGE")) ctx->frame_stage = std::atoi(v);
	if (const char* v = std::getenv("CIMBAR_HIP_WARP_TWOPASS")) ctx->warp_twopass = std::atoi(v);
	if (const char* v = std::getenv("CIMBAR_HIP_WARP_SCRATCH_MB")) { long k = std::atol(v); if (k >= 1 && k <= (1 << 20)) ctx->warp_scratch = (size_t)k << 20; }
	if (const char* v = std::getenv("CIMBAR_HIP_UNDISTORT_SCRATCH_MB")) { long k = std::atol(v); if (k >= 1 && k <= (1 << 20)) ctx->ud_scratch = (size_t)k << 20; }
	if (const char* v = std::getenv("CIMBAR_HIP_K1_STRIPS")) ctx->k1_tall = !std::strcmp(v, "tall") ? 1 : (!std::strcmp(v, "short") ? 0 : -1);
	if (const char* v = std::getenv("CIMBAR_HIP_K1_LDS_PAD")) { int k = std::atoi(v); if (k >= 0 && k <= 100000) ctx->k1_lds_pad = k; }
	if (const char* v = std::getenv("CIMBAR_HIP_FRAME_ZEROCOPY")) ctx->frame_zerocopy = std::atoi(v);
	if (const char* v = std::getenv("CIMBAR_HIP_FRAME_COPYSTREAM")) ctx->frame_copystream = std::atoi(v);
	if (const char* v = std::getenv("CIMBAR_HIP_TAIL_PARTS")) { int k = std::atoi(v); if (k >= 2 && k <= CHAIN_PARTS_MAX && k % 2 == 0) ctx->tail_parts = k; }
	for (Event& e : ctx->ev) if (e.create(hipEventDefault) != hipSuccess) return fail(CIMBAR_HIP_EHIP);
	if (ctx->d_carry.reserve(10) != hipSuccess) return fail(CIMBAR_HIP_ENOMEM);
	if (hipMemset(ctx->d_carry, 0, sizeof(float) * 10) != hipSuccess) return fail(CIMBAR_HIP_EHIP);
	if (build_tables(ctx) != 0) return fail(CIMBAR_HIP_EHIP);
	if (ctx->h_flagged.reserve(4) == hipSuccess) { ctx->h_flagged[0] = ctx->h_flagged[1] = ctx->h_flagged[2] = 0; }
	else (void)hipGetLastError();        // (only a heuristic's input: do without)
	*out = ctx;
	return CIMBAR_HIP_OK;
}

void cimbar_hip_destroy(cimbar_hip_ctx* ctx) { delete ctx; }

const char* cimbar_hip_last_error(const cimbar_hip_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int cimbar_hip_device(const cimbar_hip_ctx* ctx) { return ctx ? ctx->device : CIMBAR_HIP_EINVAL; }

int cimbar_hip_reset_ccm(cimbar_hip_ctx* ctx)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipDeviceSynchronize());   // pipelined batches in flight still carry the matrix forward
	HIPCHK(hipMemsetAsync(ctx->d_carry, 0, sizeof(float) * 10, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return 0;
}

int cimbar_hip_get_ccm(cimbar_hip_ctx* ctx, float out9[9])
{
	if (!ctx || !out9) return CIMBAR_HIP_EINVAL;
	float tmp[10];
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipDeviceSynchronize());   // whatever stream the last batch ran on
	HIPCHK(hipMemcpy(tmp, ctx->d_carry, sizeof tmp, hipMemcpyDeviceToHost));
	std::memcpy(out9, tmp, sizeof(float) * 9);
	return tmp[9] != 0.0f ? 1 : 0;
}

// CimbDecoder::update_color_correction (CimbDecoder.cpp:82-85): color_correction::update = matrix + active flag (color_correction.h:54-58)
int cimbar_hip_set_ccm(cimbar_hip_ctx* ctx, const float m9[9])
{
	if (!ctx || !m9) return CIMBAR_HIP_EINVAL;
	float tmp[10];
	std::memcpy(tmp, m9, sizeof(float) * 9);
	tmp[9] = 1.0f;
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipDeviceSynchronize());   // pipelined batches in flight still carry the old matrix forward
	HIPCHK(hipMemcpy(ctx->d_carry, tmp, sizeof tmp, hipMemcpyHostToDevice));
	return 0;
}

namespace {

// what the combined entry points add to a batch decode (combine.hip.inc); the plain entry points pass none
struct CombineArgs {
	const int* groups_in;     // host memory, n ints, or nullptr: the device groups the captures
	int min_agree, max_group; // resolved (750 / 4 for <= 0)
	int* groups_out; uint8_t* gchunks; uint32_t* gmasks; int* n_groups;
	// the stream calls: groups may span calls (n + 1 group slots, gsizes may be nullptr); groups_in is nullptr
	bool stream = false; int flush = 0; int* gsizes = nullptr;
};

// the argument checks of the combined entry points, before anything is enqueued
int check_combine(cimbar_hip_ctx* ctx, const char* who, int n, CombineArgs& cb)
{
	if (!cb.gchunks || !cb.gmasks) { ctx->err = std::string(who) + ": null gchunks / gmasks"; return CIMBAR_HIP_EINVAL; }
	if (cb.max_group > GMAX) { ctx->err = std::string(who) + ": max_group above 8"; return CIMBAR_HIP_EINVAL; }
	if (cb.max_group <= 0) cb.max_group = GROUP_MAX_DEFAULT;
	if (cb.min_agree <= 0) cb.min_agree = GROUP_AGREE_DEFAULT;
	if (cb.stream) {
		if (n == 0 && !cb.flush) { ctx->err = std::string(who) + ": n == 0 without a flush"; return CIMBAR_HIP_EINVAL; }
		if (!ctx->cstream) ctx->cstream.reset(new (std::nothrow) CombineStream);
		if (!ctx->cstream) { ctx->err = std::string(who) + ": out of memory"; return CIMBAR_HIP_EINVAL; }
		CombineStream& s = *ctx->cstream;
		if (s.max_group != 0 && (s.max_group != cb.max_group || s.min_agree != cb.min_agree)) {
			ctx->err = std::string(who) + ": min_agree_permille / max_group differ from the stream's (cimbar_hip_combine_stream_reset starts another)";
			return CIMBAR_HIP_EINVAL;
		}
		// (so a group opened without carried weights never meets a vote, and the other way round)
		const int vote = (!LEGACY && ctx->sgv_on != 0) ? 1 : 0;
		if (s.max_group != 0 && s.vote != vote) {
			ctx->err = std::string(who) + ": cimbar_hip_set_stream_colour_vote changed in mid-stream (cimbar_hip_combine_stream_reset starts another)";
			return CIMBAR_HIP_EINVAL;
		}
		s.max_group = cb.max_group; s.min_agree = cb.min_agree; s.vote = vote;
	}
	if (cb.groups_in) {
		// -1 or an id; ids start at 0 and rise by one; each id's captures contiguous and at most max_group
		int next = 0, cur = -1, cnt = 0;
		for (int k = 0; k < n; ++k) {
			const int v = cb.groups_in[k];
			if (v == -1) { cur = -1; continue; }
			if (v == cur) { if (++cnt > cb.max_group) { ctx->err = std::string(who) + ": groups_in: a group of more than max_group captures"; return CIMBAR_HIP_EINVAL; } continue; }
			if (v != next) { ctx->err = std::string(who) + ": groups_in: ids must be -1 or start at 0, rise by one and be contiguous"; return CIMBAR_HIP_EINVAL; }
			cur = v; cnt = 1; ++next;
		}
	}
	return 0;
}

int ensure_group_capacity(cimbar_hip_ctx* ctx, int n)
{
	const size_t N = (size_t)n;
	HIPCHK(ctx->d_gsym.reserve(N * NCELLS));
	HIPCHK(ctx->d_gcol.reserve(N * NCELLS));
	HIPCHK(ctx->d_gmargin.reserve(N * NCELLS));
	HIPCHK(ctx->d_grs_ok.reserve(N * ALL_BLOCKS));
	HIPCHK(ctx->d_gagree.reserve(N));
	HIPCHK(ctx->d_gdisp.reserve(N));
	HIPCHK(ctx->d_groups.reserve(N));
	HIPCHK(ctx->d_gmem.reserve(N * GMAX));
	HIPCHK(ctx->d_gcount.reserve(N));
	HIPCHK(ctx->d_groups_in.reserve(N));
	HIPCHK(ctx->d_ngroups.ensure(1));
	HIPCHK(ctx->d_gchunks.reserve(N * FRAME_BYTES));
	HIPCHK(ctx->d_gmasks.reserve(N));
	return 0;
}

// where a combined call's group chunks and masks go on the device: the caller's buffers (device outputs), or the context's staging (host
// outputs; it exists once ensure_group_capacity has run)
struct GroupOut { uint8_t* chunks; uint32_t* masks; };
GroupOut group_out(cimbar_hip_ctx* ctx, const CombineArgs& cb, int out_mem)
{
	if (out_mem == CIMBAR_HIP_MEM_DEVICE) return {cb.gchunks, cb.gmasks};
	return {ctx->d_gchunks, ctx->d_gmasks};
}

// the k_rs LIVE launches over `slots` slots of cells (combine.hip.inc, stitch.hip.inc): *n_live of them are decoded, those with a live flag, into
// d_chunks / rs_ok
void launch_live_rs(cimbar_hip_ctx* ctx, hipStream_t st, int slots, const uint8_t* sym, const uint8_t* col, uint8_t* rs_ok, const int* n_live,
                    const uint32_t* live, uint8_t* d_chunks)
{
	if constexpr (LEGACY) {
		hipLaunchKernelGGL((k_rs<CELL_BITS, false, true>), dim3((slots * ALL_BLOCKS + 3) / 4), dim3(256), 0, st, sym, ctx->tb, 0, slots, 0, d_chunks, rs_ok, 0,
		                   col, n_live, live);
	} else {
		hipLaunchKernelGGL((k_rs<4, false, true>), dim3((slots * SYM_BLOCKS + 3) / 4), dim3(256), 0, st, sym, ctx->tb, 0, slots, 0, d_chunks, rs_ok, 0,
		                   (const uint8_t*)nullptr, n_live, live);
		hipLaunchKernelGGL((k_rs<2, false, true>), dim3((slots * COL_BLOCKS + 3) / 4), dim3(256), 0, st, col, ctx->tb, 0, slots, SYM_CHUNKS, d_chunks, rs_ok,
		                   SYM_BLOCKS, (const uint8_t*)nullptr, n_live, live);
	}
}

// the groups' Reed-Solomon pass over `slots` group slots (k_rs LIVE: see combine.hip.inc), from the combined cells into d_gchunks / d_grs_ok
void launch_group_rs(cimbar_hip_ctx* ctx, hipStream_t st, int slots, uint8_t* d_gchunks)
{
	launch_live_rs(ctx, st, slots, ctx->d_gsym, ctx->d_gcol, ctx->d_grs_ok, ctx->d_ngroups, ctx->d_gdisp, d_gchunks);
}

// G1-G4 behind a batch's per-capture decode, on the same stream; reads that decode's intermediates and outputs (d_chunks / d_masks), writes
// the group outputs (d_gchunks / d_gmasks, n slots) and the context's group scratch. d_status: the capture path's extraction status (stride
// ints apart), nullptr: every capture usable. d_rgb: the frames that decode read (the colour vote takes a flooded member's means from them).
int enqueue_combine(cimbar_hip_ctx* ctx, hipStream_t st, int n, const uint8_t* d_rgb, const uint8_t* d_chunks, const uint32_t* d_masks, const int* d_status,
                    int stride, const CombineArgs& cb, int out_mem)
{
	if (int r = ensure_group_capacity(ctx, n)) return r;
	cimbar_hip_ctx::ScratchSet& cur = ctx->cur();
	// the colour vote (cimbar_hip_set_group_colour_vote) and, with the colour erasure setting on as well, the group colour retry
	const bool vote = !LEGACY && ctx->gcv_on != 0;
	if (vote) {
		HIPCHK(ctx->d_gcm.reserve((size_t)n * NCELLS));
		HIPCHK(ctx->d_gcw.reserve((size_t)n * NCELLS));
	}
	const GroupOut out = group_out(ctx, cb, out_mem);
	if (cb.groups_in) HIPCHK(hipMemcpyAsync(ctx->d_groups_in, cb.groups_in, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemsetAsync(ctx->d_gcount, 0, sizeof(int) * (size_t)n, st));
	HIPCHK(hipMemsetAsync(ctx->d_gdisp, 0, sizeof(uint32_t) * (size_t)n, st));
	if (!cb.groups_in && n > 1)
		hipLaunchKernelGGL(k_group_agree, dim3(n - 1), dim3(256), 0, st, cur.d_symbols, cur.d_colors, n, ctx->d_gagree);
	hipLaunchKernelGGL(k_group_walk, dim3(1), dim3(64), 0, st, ctx->d_gagree, n, d_status, stride, cb.groups_in ? ctx->d_groups_in : (const int*)nullptr,
	                   cb.min_agree, cb.max_group, ctx->d_groups, ctx->d_gmem, ctx->d_gcount, ctx->d_ngroups);
	hipLaunchKernelGGL(k_group_cells, dim3(GC_BLOCKS, n), dim3(256), 0, st, cur.d_plane, ctx->tb, cur.d_symbols, cur.d_colors, cur.d_drift, cur.d_flood,
	                   ctx->d_gmem, ctx->d_gcount, ctx->d_ngroups, ctx->d_gsym, ctx->d_gcol, ctx->d_gmargin, ctx->d_gdisp);
	if (vote)
		hipLaunchKernelGGL(k_group_colour, dim3(n), dim3(256), 0, st, d_rgb, cur.d_cellmean, ctx->tb, cur.d_colors, cur.d_drift, cur.d_flood, cur.d_ccm_used,
		                   ctx->d_gmem, ctx->d_gcount, ctx->d_ngroups, ctx->d_gdisp, ctx->d_gcol, ctx->d_gcm, ctx->d_gcw);
	launch_group_rs(ctx, st, n, out.chunks);
	hipLaunchKernelGGL(k_group_end, dim3(n), dim3(256), 0, st, ctx->d_gsym, ctx->d_gmargin, ctx->tb, ctx->d_gmem, ctx->d_gcount, ctx->d_ngroups, ctx->d_grs_ok,
	                   d_chunks, d_masks, ctx->d_gdisp, out.chunks, out.masks, (!LEGACY && ctx->er_sym > 0) ? 1 : 0, erasure_max(ctx));
	if (vote && ctx->ec_margin > 0)
		hipLaunchKernelGGL(k_group_colour_retry, dim3(n), dim3(256), 0, st, ctx->d_gcol, ctx->d_gcm, ctx->tb, ctx->d_gcount, ctx->d_ngroups, ctx->d_gdisp,
		                   ctx->d_grs_ok, out.chunks, out.masks, ctx->ec_margin, colour_erasure_max(ctx));
	HIPCHK(hipGetLastError());
	ctx->gcv_valid = vote;
	ctx->gcv_stream_n = -1;
	return 0;
}

// the stream calls' buffers: the carry store (fixed size, allocated by the first stream call) and the n + 1 group slots
int ensure_stream_capacity(cimbar_hip_ctx* ctx, int n)
{
	if (int r = ensure_group_capacity(ctx, n + 1)) return r;
	CombineStream& s = *ctx->cstream;
	HIPCHK(s.ev_last.create());
	HIPCHK(s.symbols.ensure(CARRY_SLOTS * CS_CELLS));
	HIPCHK(s.colors.ensure(CARRY_SLOTS * CS_CELLS));
	HIPCHK(s.drift.ensure(CARRY_SLOTS * CS_DRIFT));
	HIPCHK(s.plane.ensure(CARRY_SLOTS * CS_PLANE));
	HIPCHK(s.chunks.ensure(CARRY_SLOTS * CS_CHUNKS));
	HIPCHK(s.flood.ensure(CARRY_SLOTS));
	HIPCHK(s.masks.ensure(CARRY_SLOTS));
	if (!s.words) { HIPCHK(s.words.ensure(2)); HIPCHK(hipMemset(s.words, 0, sizeof(int) * 2)); }
	HIPCHK(s.gsizes.reserve((size_t)n + 1));
	if (s.vote) {   // (a context that never turns the stream vote on pays nothing)
		HIPCHK(s.weights.ensure(CARRY_SLOTS * CS_WEIGHTS));
		HIPCHK(ctx->d_gcm.reserve(((size_t)n + 1) * NCELLS));
		HIPCHK(ctx->d_gcw.reserve((size_t)(n > 0 ? n : 1) * NCELLS));
	}
	return 0;
}

// The stream calls' G1-G5 behind a batch's per-capture decode (none for n == 0), on the same stream and behind the stream call before: the
// virtual batch is the carry store's members followed by the n captures. Group outputs have n + 1 slots. d_rgb: the frames that decode read.
// The colour vote here is the stream's own setting (cimbar_hip_set_stream_colour_vote, sampled by check_combine), never the plain calls'; with
// it the vote runs over the virtual batch, with the colour erasure setting on as well the group colour retry, and the weights of the members
// that stay open are carried. Every reader of the carried weights is launched in front of their writer; nothing waits for the host.
int enqueue_combine_stream(cimbar_hip_ctx* ctx, hipStream_t st, int n, const uint8_t* d_rgb, const uint8_t* d_chunks, const uint32_t* d_masks,
                           const int* d_status, int stride, const CombineArgs& cb, int out_mem)
{
	if (int r = ensure_stream_capacity(ctx, n)) return r;
	CombineStream& s = *ctx->cstream;
	const bool vote = !LEGACY && s.vote != 0;
	ctx->gcv_valid = vote;
	ctx->gcv_stream_n = vote ? n : -1;
	cimbar_hip_ctx::ScratchSet& cur = ctx->cur();
	const CarryStore cs = s.store();
	const int slots = n + 1;
	const GroupOut out = group_out(ctx, cb, out_mem);
	int* d_gsizes = (out_mem == CIMBAR_HIP_MEM_DEVICE && cb.gsizes) ? cb.gsizes : s.gsizes;
	if (s.used) HIPCHK(hipStreamWaitEvent(st, s.ev_last, 0));
	s.used = true;
	HIPCHK(hipMemsetAsync(ctx->d_gcount, 0, sizeof(int) * (size_t)slots, st));
	HIPCHK(hipMemsetAsync(ctx->d_gdisp, 0, sizeof(uint32_t) * (size_t)slots, st));
	if (n > 0)
		hipLaunchKernelGGL(k_group_agree_stream, dim3(n), dim3(256), 0, st, cur.d_symbols, cur.d_colors, n, cs, ctx->d_gagree);
	hipLaunchKernelGGL(k_group_walk_stream, dim3(1), dim3(64), 0, st, ctx->d_gagree, n, d_status, stride, cb.min_agree, cb.max_group, cb.flush ? 1 : 0, cs,
	                   ctx->d_groups, ctx->d_gmem, ctx->d_gcount, ctx->d_ngroups, s.words + 1);
	hipLaunchKernelGGL(k_group_cells_stream, dim3(GC_BLOCKS, slots), dim3(256), 0, st, cur.d_plane, ctx->tb, cur.d_symbols, cur.d_colors, cur.d_drift,
	                   cur.d_flood, ctx->d_gmem, ctx->d_gcount, ctx->d_ngroups, ctx->d_gsym, ctx->d_gcol, ctx->d_gmargin, ctx->d_gdisp, cs);
	if (vote)
		hipLaunchKernelGGL(k_group_colour_stream, dim3(slots), dim3(256), 0, st, d_rgb, cur.d_cellmean, ctx->tb, cur.d_colors, cur.d_drift, cur.d_flood,
		                   cur.d_ccm_used, ctx->d_gmem, ctx->d_gcount, ctx->d_ngroups, ctx->d_gdisp, ctx->d_gcol, ctx->d_gcm, ctx->d_gcw, cs);
	launch_group_rs(ctx, st, slots, out.chunks);
	hipLaunchKernelGGL(k_group_end_stream, dim3(slots), dim3(256), 0, st, ctx->d_gsym, ctx->d_gmargin, ctx->tb, ctx->d_gmem, ctx->d_gcount, ctx->d_ngroups,
	                   ctx->d_grs_ok, d_chunks, d_masks, ctx->d_gdisp, out.chunks, out.masks, (!LEGACY && ctx->er_sym > 0) ? 1 : 0, erasure_max(ctx), cs, d_gsizes);
	if (vote && ctx->ec_margin > 0)
		hipLaunchKernelGGL(k_group_colour_retry, dim3(slots), dim3(256), 0, st, ctx->d_gcol, ctx->d_gcm, ctx->tb, ctx->d_gcount, ctx->d_ngroups, ctx->d_gdisp,
		                   ctx->d_grs_ok, out.chunks, out.masks, ctx->ec_margin, colour_erasure_max(ctx));
	hipLaunchKernelGGL(k_group_carry, dim3(CARRY_ARRAYS * CARRY_PARTS, CARRY_SLOTS), dim3(256), 0, st, cur.d_plane, cur.d_symbols, cur.d_colors, cur.d_drift,
	                   cur.d_flood, d_chunks, d_masks, ctx->d_gmem, ctx->d_ngroups, s.words + 1, ctx->d_groups, cs);
	if (vote)
		hipLaunchKernelGGL(k_group_carry_weights, dim3(CW_BLOCKS, CARRY_SLOTS), dim3(256), 0, st, d_rgb, cur.d_cellmean, ctx->tb, cur.d_drift, cur.d_flood,
		                   cur.d_ccm_used, ctx->d_gmem, ctx->d_ngroups, s.words + 1, cs);
	HIPCHK(hipGetLastError());
	return 0;
}

// the end of a stream call: finish_batch with n + 1 group slots and gsizes, and the event the next stream call waits for
int64_t finish_stream(cimbar_hip_ctx* ctx, hipStream_t st, int n, uint8_t* chunks, uint32_t* masks, const uint8_t* d_chunks, const uint32_t* d_masks,
                      int out_mem, const CombineArgs& cb)
{
	CombineStream& s = *ctx->cstream;
	const hipMemcpyKind kind = out_mem == CIMBAR_HIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
	const size_t slots = (size_t)n + 1;
	int ng = 0;
	if (cb.groups_out && n > 0) HIPCHK(hipMemcpyAsync(cb.groups_out, ctx->d_groups, sizeof(int) * (size_t)n, kind, st));
	if (out_mem == CIMBAR_HIP_MEM_DEVICE) {
		if (cb.n_groups) HIPCHK(hipMemcpyAsync(cb.n_groups, ctx->d_ngroups, sizeof(int), kind, st));
	} else {
		if (n > 0) {
			HIPCHK(hipMemcpyAsync(chunks, d_chunks, (size_t)n * FRAME_BYTES, hipMemcpyDeviceToHost, st));
			HIPCHK(hipMemcpyAsync(masks, d_masks, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
		}
		HIPCHK(hipMemcpyAsync(cb.gchunks, ctx->d_gchunks, slots * FRAME_BYTES, hipMemcpyDeviceToHost, st));
		HIPCHK(hipMemcpyAsync(cb.gmasks, ctx->d_gmasks, sizeof(uint32_t) * slots, hipMemcpyDeviceToHost, st));
		if (cb.gsizes) HIPCHK(hipMemcpyAsync(cb.gsizes, s.gsizes, sizeof(int) * slots, hipMemcpyDeviceToHost, st));
		HIPCHK(hipMemcpyAsync(&ng, ctx->d_ngroups, sizeof(int), hipMemcpyDeviceToHost, st));
	}
	HIPCHK(hipEventRecord(s.ev_last, st));
	ctx->grp_valid = true;
	if (out_mem == CIMBAR_HIP_MEM_DEVICE) return 0;
	HIPCHK(hipStreamSynchronize(st));
	if (cb.n_groups) *cb.n_groups = ng;
	return ng;
}

// the stage timers of the last enqueue() with timing on, once its events are complete
int read_stage_times(cimbar_hip_ctx* ctx)
{
	for (int k = 0; k < cimbar_hip_ctx::NSTAGE; ++k) HIPCHK(hipEventElapsedTime(&ctx->stage_ms[k], ctx->ev[k], ctx->ev[k + 1]));
	return 0;
}

// the end of a batch call: device outputs are enqueued (group ids and count included) and 0 returned; host outputs are copied back, then
// the call synchronises and returns the good bytes over the batch, or with `cb` the group count
int64_t finish_batch(cimbar_hip_ctx* ctx, hipStream_t st, int n, uint8_t* chunks, uint32_t* masks, const uint8_t* d_chunks, const uint32_t* d_masks,
                     int out_mem, const CombineArgs* cb)
{
	const hipMemcpyKind kind = out_mem == CIMBAR_HIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
	if (cb && cb->groups_out) HIPCHK(hipMemcpyAsync(cb->groups_out, ctx->d_groups, sizeof(int) * (size_t)n, kind, st));
	if (out_mem == CIMBAR_HIP_MEM_DEVICE) {
		if (cb && cb->n_groups) HIPCHK(hipMemcpyAsync(cb->n_groups, ctx->d_ngroups, sizeof(int), kind, st));
		if (cb) ctx->grp_valid = true;
		return 0;
	}
	int ng = 0;
	HIPCHK(hipMemcpyAsync(chunks, d_chunks, (size_t)n * FRAME_BYTES, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(masks, d_masks, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
	if (cb) {
		HIPCHK(hipMemcpyAsync(cb->gchunks, ctx->d_gchunks, (size_t)n * FRAME_BYTES, hipMemcpyDeviceToHost, st));
		HIPCHK(hipMemcpyAsync(cb->gmasks, ctx->d_gmasks, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
		HIPCHK(hipMemcpyAsync(&ng, ctx->d_ngroups, sizeof(int), hipMemcpyDeviceToHost, st));
	}
	HIPCHK(hipStreamSynchronize(st));
	if (cb) {
		ctx->grp_valid = true;
		if (cb->n_groups) *cb->n_groups = ng;
		return ng;
	}
	// aligned_stream::tellp() summed over the batch: 625 bytes per delivered chunk (aligned_stream.h:29-32)
	unsigned long long total = 0;
	for (int f = 0; f < n; ++f) total += (unsigned long long)CHUNK * (unsigned)__builtin_popcount(masks[f] & ((1u << CHUNKS) - 1u));
	return (int64_t)total;
}

// ------------------------------------------------------------------------------------------------ torn-capture stitching (stitch.hip.inc)
struct StitchArgs {
	int axis, min_agree, min_band;
	uint8_t* schunks; uint32_t* smasks; int32_t* tears;   // 2 rows slots; rows x 4 ints (may be nullptr)
	std::vector<int32_t> h_tears;                         // host outputs: where the tear records land when the caller wants none
	bool stream = false;                                  // a stream call: n rows, row 0 against the carried capture; else n - 1
	int strips = 1;                                       // cimbar_hip_set_stitch_strips as the call found it (check_stitch)
	int er_sym = 0, er_col = 0;                           // cimbar_hip_set_stitch_erasure as the call found it: the armed retries' thresholds (0: not run)
	int rows(int n) const { return stream ? n : n - 1; }
};

// the argument checks of the stitched entry points, before anything is enqueued
int check_stitch(cimbar_hip_ctx* ctx, const char* who, int n, StitchArgs& sa)
{
	if (sa.axis != 0 && sa.axis != 1) { ctx->err = std::string(who) + ": axis must be 0 (grid rows) or 1 (grid columns)"; return CIMBAR_HIP_EINVAL; }
	if (sa.min_band > stitch_lines(sa.axis)) { ctx->err = std::string(who) + ": min_band above the lines of the axis"; return CIMBAR_HIP_EINVAL; }
	if (sa.rows(n) > 0 && (!sa.schunks || !sa.smasks)) { ctx->err = std::string(who) + ": null schunks / smasks"; return CIMBAR_HIP_EINVAL; }
	if (sa.min_agree <= 0) sa.min_agree = STITCH_AGREE_DEFAULT;
	if (sa.min_band <= 0) sa.min_band = STITCH_BAND_DEFAULT;
	sa.strips = ctx->stitch_strips;
	// (the stream calls carry cells, not planes or means: the retry does not reach them)
	const bool er = !LEGACY && ctx->stitch_er && !sa.stream;
	sa.er_sym = er ? ctx->er_sym : 0;
	sa.er_col = er ? ctx->ec_margin : 0;
	return 0;
}

int ensure_stitch_capacity(cimbar_hip_ctx* ctx, int rows, int strips, bool er_sym, bool er_col)
{
	const size_t P = (size_t)rows, S = 2 * P;
	if (er_sym) HIPCHK(ctx->d_sdist.reserve(S * NCELLS));
	if (er_col) HIPCHK(ctx->d_smargin.reserve(S * NCELLS));
	if (er_sym || er_col) HIPCHK(ctx->d_sworked.reserve(2 * S));
	if (strips > 1) {
		HIPCHK(ctx->d_sstrips.reserve(P * STITCH_SMAX * 4));
		HIPCHK(ctx->d_sstrip_lines.reserve(P * STITCH_SMAX * STITCH_LMAX));
	}
	HIPCHK(ctx->d_ssym.reserve(S * NCELLS));
	HIPCHK(ctx->d_scol.reserve(S * NCELLS));
	HIPCHK(ctx->d_srs_ok.reserve(S * ALL_BLOCKS));
	HIPCHK(ctx->d_slive.reserve(S));
	HIPCHK(ctx->d_stears.reserve(P * 4));
	HIPCHK(ctx->d_slines.reserve(P * STITCH_LMAX));
	HIPCHK(ctx->d_sslots.ensure(1));
	HIPCHK(ctx->d_schunks.reserve(S * FRAME_BYTES));
	HIPCHK(ctx->d_smasks.reserve(S));
	return 0;
}

// the start of a stitched-stream call, in front of its per-capture decode: the carry store (allocated by the first such call, nothing
// carried) and the wait that puts the whole call behind the stitched-stream call before, whatever their streams
int begin_stitch_stream(cimbar_hip_ctx* ctx, hipStream_t st)
{
	if (!ctx->sstream) ctx->sstream = std::make_unique<StitchStream>();
	StitchStream& s = *ctx->sstream;
	HIPCHK(s.ev_last.create());
	HIPCHK(s.symbols.ensure((size_t)2 * SS_CELLS));
	HIPCHK(s.colors.ensure((size_t)2 * SS_CELLS));
	if (!s.usable) { HIPCHK(s.usable.ensure(2)); HIPCHK(hipMemset(s.usable, 0, sizeof(uint32_t) * 2)); }
	if (s.used) HIPCHK(hipStreamWaitEvent(st, s.ev_last, 0));
	return 0;
}

// S1, the Reed-Solomon pass over the 2 rows slots (launch_live_rs: the k_rs LIVE instances of the group decode, fed from the stitch scratch) and S2, behind
// a batch's per-capture decode on the same stream (rows > 0: n - 1 pairs, a stream call n rows). Reads that decode's symbols and colours; writes the
// caller's buffers (device outputs) or the context's staging, whose copies back to the host are enqueued here as well. d_status as for enqueue_combine.
// A stream call (after begin_stitch_stream): S1 reads the carried capture from one slot and leaves its last capture in the other.
int enqueue_stitch(cimbar_hip_ctx* ctx, hipStream_t st, int n, const uint8_t* d_frames, const int* d_status, int stride, StitchArgs& sa, int out_mem)
{
	const int pairs = sa.rows(n), slots = 2 * pairs;
	if (int r = ensure_stitch_capacity(ctx, pairs, sa.strips, sa.er_sym > 0, sa.er_col > 0)) return r;
	cimbar_hip_ctx::ScratchSet& cur = ctx->cur();
	const bool dev = out_mem == CIMBAR_HIP_MEM_DEVICE;
	uint8_t* d_out = dev ? sa.schunks : ctx->d_schunks.get();
	uint32_t* d_om = dev ? sa.smasks : ctx->d_smasks.get();
	HIPCHK(hipMemsetAsync(ctx->d_sslots, 0, sizeof(int), st));
	const uint16_t* strip_width = ctx->tb_stitch_width + (size_t)(sa.axis * STITCH_SMAX + sa.strips - 1) * STITCH_SMAX * 128;
	if (sa.stream) {
		StitchStream& s = *ctx->sstream;
		if (sa.strips > 1)
			hipLaunchKernelGGL(k_stitch_pairs_strips_stream, dim3(pairs), dim3(256), 0, st, cur.d_symbols, cur.d_colors, n, d_status, stride,
			                   ctx->tb_stitch_line, strip_width, sa.axis, sa.strips, sa.min_agree, sa.min_band, ctx->d_stears, ctx->d_slines, ctx->d_sstrips,
			                   ctx->d_sstrip_lines, ctx->d_slive, ctx->d_sslots, ctx->d_ssym, ctx->d_scol, s.carry());
		else
			hipLaunchKernelGGL(k_stitch_pairs_stream, dim3(pairs), dim3(256), 0, st, cur.d_symbols, cur.d_colors, n, d_status, stride, ctx->tb_stitch_line,
			                   sa.axis, sa.min_agree, sa.min_band, ctx->d_stears, ctx->d_slines, ctx->d_slive, ctx->d_sslots, ctx->d_ssym, ctx->d_scol, s.carry());
		HIPCHK(hipGetLastError());
		s.cur ^= 1;   // (the slot that launch fills)
		s.carried = true;
	} else if (sa.strips > 1)
		hipLaunchKernelGGL(k_stitch_pairs_strips, dim3(pairs), dim3(256), 0, st, cur.d_symbols, cur.d_colors, n, d_status, stride, ctx->tb_stitch_line,
		                   strip_width, sa.axis, sa.strips, sa.min_agree, sa.min_band, ctx->d_stears, ctx->d_slines, ctx->d_sstrips, ctx->d_sstrip_lines,
		                   ctx->d_slive, ctx->d_sslots, ctx->d_ssym, ctx->d_scol);
	else
		hipLaunchKernelGGL(k_stitch_pairs, dim3(pairs), dim3(256), 0, st, cur.d_symbols, cur.d_colors, n, d_status, stride, ctx->tb_stitch_line, sa.axis,
		                   sa.min_agree, sa.min_band, ctx->d_stears, ctx->d_slines, ctx->d_slive, ctx->d_sslots, ctx->d_ssym, ctx->d_scol);
	launch_live_rs(ctx, st, slots, ctx->d_ssym, ctx->d_scol, ctx->d_srs_ok, ctx->d_sslots, ctx->d_slive, d_out);
	hipLaunchKernelGGL(k_stitch_end, dim3(slots), dim3(256), 0, st, ctx->d_slive, ctx->d_srs_ok, d_out, d_om);
	// opt-in erasure retry of the chunks a slot's mask lacks (cimbar_hip_set_stitch_erasure): the symbol retry, then the colour retry, each only
	// where its own erasure setting is on; they read the two captures' intermediates of the per-capture decode and write the slot's chunks and mask
	if (sa.er_sym > 0)
		hipLaunchKernelGGL(k_stitch_erasure, dim3(slots), dim3(256), 0, st, cur.d_plane, ctx->tb, cur.d_drift, cur.d_flood, ctx->tb_stitch_line, sa.axis,
		                   sa.strips, ctx->d_stears, ctx->d_sstrips, ctx->d_slive, ctx->d_ssym, ctx->d_srs_ok, d_out, d_om, ctx->d_sdist, ctx->d_sworked,
		                   sa.er_sym, erasure_max(ctx));
	if (sa.er_col > 0)
		hipLaunchKernelGGL(k_stitch_colour_erasure, dim3(slots), dim3(256), 0, st, d_frames, cur.d_cellmean, ctx->tb, cur.d_drift, cur.d_flood,
		                   cur.d_ccm_used, ctx->tb_stitch_line, sa.axis, sa.strips, ctx->d_stears, ctx->d_sstrips, ctx->d_slive, ctx->d_scol, ctx->d_srs_ok,
		                   d_out, d_om, ctx->d_smargin, ctx->d_sworked + slots, sa.er_col, colour_erasure_max(ctx));
	HIPCHK(hipGetLastError());
	if (dev) {
		if (sa.tears) HIPCHK(hipMemcpyAsync(sa.tears, ctx->d_stears, sizeof(int32_t) * 4 * (size_t)pairs, hipMemcpyDeviceToDevice, st));
	} else {
		if (!sa.tears) { sa.h_tears.resize((size_t)pairs * 4); sa.tears = sa.h_tears.data(); }
		HIPCHK(hipMemcpyAsync(sa.schunks, d_out, (size_t)slots * FRAME_BYTES, hipMemcpyDeviceToHost, st));
		HIPCHK(hipMemcpyAsync(sa.smasks, d_om, sizeof(uint32_t) * (size_t)slots, hipMemcpyDeviceToHost, st));
		HIPCHK(hipMemcpyAsync(sa.tears, ctx->d_stears, sizeof(int32_t) * 4 * (size_t)pairs, hipMemcpyDeviceToHost, st));
	}
	return 0;
}

// the end of a stitched call: finish_batch for the per-capture outputs; host outputs: the candidate pairs, read from the tear records.
// A stream call records the event the next one waits for, behind everything it enqueued.
int64_t finish_stitched(cimbar_hip_ctx* ctx, hipStream_t st, int n, uint8_t* chunks, uint32_t* masks, const uint8_t* d_chunks, const uint32_t* d_masks,
                        int out_mem, const StitchArgs& sa)
{
	const int64_t r = finish_batch(ctx, st, n, chunks, masks, d_chunks, d_masks, out_mem, nullptr);
	if (r < 0) return r;
	ctx->stitch_n = n;
	ctx->stitch_rows = sa.rows(n);
	ctx->stitch_axis = sa.axis;
	ctx->stitch_S = sa.strips;
	ctx->stitch_er_ran = sa.rows(n) > 0 ? (sa.er_sym > 0 ? 1 : 0) | (sa.er_col > 0 ? 2 : 0) : 0;
	if (sa.stream) {
		HIPCHK(hipEventRecord(ctx->sstream->ev_last, st));
		ctx->sstream->used = true;
	}
	if (out_mem == CIMBAR_HIP_MEM_DEVICE) return 0;
	int64_t cand = 0;
	for (int k = 0; k < sa.rows(n); ++k) cand += sa.tears[(size_t)k * 4] >= 0;
	return cand;
}

// what a capture entry point has and a frame one has not: the captures' size and format as the caller gave them, where their extraction
// status goes (may be nullptr), and -- resolved by begin_decode -- the format the kernels take and a capture's bytes
struct CaptureIn { unsigned width, height; int format; int* status; int fmt = 0; size_t cbytes = 0; };

// The one driver of the plain / combined / combined-stream / stitched / stitched-stream calls, over frames (cap == nullptr: `img` is n frames)
// or captures; defined behind the capture front end it drives. `pad`: decode_frame's image larger than the frame.
int64_t decode_impl(cimbar_hip_ctx* ctx, CaptureIn* cap, const uint8_t* img, int n, int img_mem, int preprocess, int color_correction, uint8_t* chunks,
                    uint32_t* masks, int out_mem, void* hip_stream, CombineArgs* cb, StitchArgs* sa = nullptr, const PadSource* pad = nullptr);

}  // namespace

int64_t cimbar_hip_decode_batch(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess,
                                int color_correction, uint8_t* chunks, uint32_t* masks, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return decode_impl(ctx, nullptr, rgb, n, rgb_mem, should_preprocess, color_correction, chunks, masks, out_mem, hip_stream, nullptr);
}

int64_t cimbar_hip_decode_batch_combined(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                         const int* groups_in, int min_agree_permille, int max_group, uint8_t* chunks, uint32_t* masks,
                                         int* groups_out, uint8_t* gchunks, uint32_t* gmasks, int* n_groups, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	CombineArgs cb{groups_in, min_agree_permille, max_group, groups_out, gchunks, gmasks, n_groups};
	return decode_impl(ctx, nullptr, rgb, n, rgb_mem, should_preprocess, color_correction, chunks, masks, out_mem, hip_stream, &cb);
}

int64_t cimbar_hip_decode_batch_combined_stream(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                                int min_agree_permille, int max_group, int flush, uint8_t* chunks, uint32_t* masks, int* groups_out,
                                                uint8_t* gchunks, uint32_t* gmasks, int* gsizes, int* n_groups, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	CombineArgs cb{nullptr, min_agree_permille, max_group, groups_out, gchunks, gmasks, n_groups, true, flush, gsizes};
	return decode_impl(ctx, nullptr, rgb, n, rgb_mem, should_preprocess, color_correction, chunks, masks, out_mem, hip_stream, &cb);
}

int64_t cimbar_hip_decode_batch_stitched(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                         int axis, int min_agree_permille, int min_band, uint8_t* chunks, uint32_t* masks, uint8_t* schunks,
                                         uint32_t* smasks, int32_t* tears, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	StitchArgs sa{axis, min_agree_permille, min_band, schunks, smasks, tears, {}};
	return decode_impl(ctx, nullptr, rgb, n, rgb_mem, should_preprocess, color_correction, chunks, masks, out_mem, hip_stream, nullptr, &sa);
}

int64_t cimbar_hip_decode_batch_stitched_stream(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                                int axis, int min_agree_permille, int min_band, uint8_t* chunks, uint32_t* masks, uint8_t* schunks,
                                                uint32_t* smasks, int32_t* tears, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	StitchArgs sa{axis, min_agree_permille, min_band, schunks, smasks, tears, {}, true};
	return decode_impl(ctx, nullptr, rgb, n, rgb_mem, should_preprocess, color_correction, chunks, masks, out_mem, hip_stream, nullptr, &sa);
}

// wait for the stitched-stream calls issued so far and forget the carry: the next one's row 0 has no partner
int cimbar_hip_stitch_stream_reset(cimbar_hip_ctx* ctx)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (!ctx->sstream) return 0;
	StitchStream& s = *ctx->sstream;
	HIPCHK(hipSetDevice(ctx->device));
	if (s.used) HIPCHK(hipEventSynchronize(s.ev_last));
	if (s.usable) HIPCHK(hipMemset(s.usable, 0, sizeof(uint32_t) * 2));
	s.carried = false;
	return 0;
}

// drop the open group and the fixed parameters: the next stream call starts a stream of its own
int cimbar_hip_combine_stream_reset(cimbar_hip_ctx* ctx)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (!ctx->cstream) return 0;
	CombineStream& s = *ctx->cstream;
	HIPCHK(hipSetDevice(ctx->device));
	if (s.used) HIPCHK(hipEventSynchronize(s.ev_last));
	if (s.words) HIPCHK(hipMemset(s.words, 0, sizeof(int) * 2));
	s.min_agree = s.max_group = 0;
	return 0;
}

int cimbar_hip_decode_batch_pipelined(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int should_preprocess, int color_correction,
                                      uint8_t* chunks, uint32_t* masks, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (!rgb || !chunks || !masks || n <= 0) { ctx->err = "decode_batch_pipelined: null buffer or n <= 0"; return CIMBAR_HIP_EINVAL; }
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t st = (hipStream_t)hip_stream;
	if (ctx->flood_verify) HIPCHK(hipDeviceSynchronize());   // the verify buffers are one set per context: batches do not overlap in this mode
	rotate_scratch_sets(ctx);
	const int set = ctx->pipe_set;
	hipStream_t own = ctx->pstream[set];
	// the frames are whatever `hip_stream` has produced up to here
	HIPCHK(hipEventRecord(ctx->ev_pk1[set], st));
	HIPCHK(hipStreamWaitEvent(own, ctx->ev_pk1[set], 0));
	// (this set's intermediates belong to the batch issued pipe_depth calls ago on the same stream: stream order keeps them apart)
	if (int r = ensure_capacity(ctx, n)) return r;
	ChainArgs ca;
	ca.d_rgb = rgb; ca.n = n; ca.pre = should_preprocess; ca.cc = color_correction;
	ca.d_chunks = chunks; ca.d_masks = masks;
	ca.pipe = true;
	return enqueue(ctx, own, ca);
}

int cimbar_hip_pipeline_depth(const cimbar_hip_ctx* ctx) { return ctx ? ctx->pipe_depth : CIMBAR_HIP_EINVAL; }

int cimbar_hip_pipeline_wait(cimbar_hip_ctx* ctx, void* hip_stream, int keep_newest)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t st = (hipStream_t)hip_stream;
	// batch j's colour pass waits for batch j-1's end, so the end of one batch implies the end of every earlier one
	if (keep_newest < 0) keep_newest = 0;
	if (keep_newest >= ctx->pipe_depth) return 0;
	const int target = (ctx->pipe_set + ctx->pipe_depth - keep_newest) % ctx->pipe_depth;
	if (ctx->pipe_used[target]) HIPCHK(hipStreamWaitEvent(st, ctx->ev_pdone[target], 0));
	// (exchanges ride on their batches' streams, one behind the other per stream, but the streams are independent: every covered set's exchange is waited for)
	for (int back = keep_newest; back < ctx->pipe_depth; ++back) {
		const int t = (ctx->pipe_set + ctx->pipe_depth - back) % ctx->pipe_depth;
		if (ctx->pipe_used[t] && ctx->pipe_gathered[t]) HIPCHK(hipStreamWaitEvent(st, ctx->ev_pgather[t], 0));
	}
	return 0;
}

int64_t cimbar_hip_decode_plain_batch(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess,
                                      int color_correction, uint8_t* bytes, uint8_t* block_ok, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (!rgb || !bytes || n <= 0) { ctx->err = "decode_plain_batch: null buffer or n <= 0"; return CIMBAR_HIP_EINVAL; }
	if (ctx->er_sym > 0) { ctx->err = "decode_plain_batch: erasure decoding is on (cimbar_hip_set_erasure_decode); the plain stream has no chunk mask to extend"; return CIMBAR_HIP_EINVAL; }
	if (ctx->ec_margin > 0) { ctx->err = "decode_plain_batch: colour erasure decoding is on (cimbar_hip_set_colour_erasure_decode); the plain stream has no chunk mask to extend"; return CIMBAR_HIP_EINVAL; }
	hipStream_t st;
	if (int r = begin_call(ctx, "decode_plain_batch", "rgb_mem", rgb_mem, "out_mem", out_mem, hip_stream, &st)) return r;
	if (int r = ensure_capacity(ctx, n)) return r;
	ChainArgs ca;
	if (int r = stage_input(ctx, st, ctx->d_rgb, rgb, (size_t)n * FRAME_RGB, rgb_mem, &ca.d_rgb)) return r;
	uint8_t* d_bytes = out_mem == CIMBAR_HIP_MEM_DEVICE ? bytes : ctx->d_chunks;
	ca.n = n; ca.pre = should_preprocess; ca.cc = color_correction;
	ca.d_chunks = d_bytes; ca.d_masks = ctx->d_masks;
	ca.plain = 1;
	if (int r = enqueue(ctx, st, ca)) return r;
	if (block_ok)
		HIPCHK(hipMemcpyAsync(block_ok, ctx->cur().d_rs_ok, (size_t)n * ALL_BLOCKS, out_mem == CIMBAR_HIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
	if (out_mem == CIMBAR_HIP_MEM_DEVICE) return 0;
	HIPCHK(hipMemcpyAsync(bytes, d_bytes, (size_t)n * FRAME_BYTES, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return (int64_t)n * FRAME_BYTES;   // what tellp() of the output stream advanced by: every block is written, good or zeroed
}

// one frame through the batch entry point on the context's own stream, complete on return (every image size; what the asynchronous call falls back to)
int cimbar_hip_decode_frame_sync(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, size_t stride,
                                 int should_preprocess, int color_correction, uint8_t* chunks, uint32_t* good_mask)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (!rgb || !chunks || !good_mask) { ctx->err = "decode_frame: null buffer"; return CIMBAR_HIP_EINVAL; }
	if (stride != 0 && stride < (size_t)width * 3) { ctx->err = "decode_frame: stride < width*3"; return CIMBAR_HIP_EINVAL; }
	if (width < (unsigned)IMG_W || height < (unsigned)IMG_H) {
		// CimbReader::_good == false (CimbReader.cpp:119): no cell is read, Decoder::do_decode flushes all-zero symbol and colour buffers through
		// Reed-Solomon -- all-zero blocks are valid codewords -- and aligned_stream delivers every chunk: the reference returns the full byte
		// count with chunks of zeros (which any fountain sink then drops as malformed). Kept as it is; no device work.
		std::memset(chunks, 0, FRAME_BYTES);
		*good_mask = (1u << CHUNKS) - 1u;
		return FRAME_BYTES;
	}
	if (width > (unsigned)IMG_W || height > (unsigned)IMG_H) {
		// a larger image: the grid sits _gridPadding pixels in (CimbReader.cpp:112-117); see k1_padded.hip.inc
		if ((uint64_t)width * height * 3 >= (1ull << 31)) { ctx->err = "decode_frame: image of 2 GiB or more"; return CIMBAR_HIP_EDIM; }
		HIPCHK(hipSetDevice(ctx->device));
		const size_t row = (size_t)width * 3, bytes = row * height;
		HIPCHK(ctx->d_ex_in.reserve(bytes));
		HIPCHK(ctx->d_rgb.reserve((size_t)FRAME_RGB));
		HIPCHK(hipDeviceSynchronize());   // (single-image edge path: nothing of an earlier call may still be reading the scratch)
		HIPCHK(hipMemcpy2D(ctx->d_ex_in, row, rgb, stride ? stride : row, row, height, hipMemcpyHostToDevice));
		const unsigned ex = width - (unsigned)IMG_W, ey = height - (unsigned)IMG_H;
		const PadSource pad{ctx->d_ex_in, (int)width, (int)height, (int)((ex < ey ? ex : ey) / 2)};
		return (int)decode_impl(ctx, nullptr, ctx->d_rgb, 1, CIMBAR_HIP_MEM_DEVICE, should_preprocess, color_correction, chunks, good_mask, CIMBAR_HIP_MEM_HOST,
		                        nullptr, nullptr, nullptr, &pad);
	}
	if (stride == (size_t)IMG_W * 3 || stride == 0)
		return (int)cimbar_hip_decode_batch(ctx, rgb, 1, CIMBAR_HIP_MEM_HOST, should_preprocess, color_correction, chunks, good_mask, CIMBAR_HIP_MEM_HOST, nullptr);
	std::vector<uint8_t> packed(FRAME_RGB);
	for (int y = 0; y < IMG_H; ++y) std::memcpy(packed.data() + (size_t)y * IMG_W * 3, rgb + (size_t)y * stride, (size_t)IMG_W * 3);
	return (int)cimbar_hip_decode_batch(ctx, packed.data(), 1, CIMBAR_HIP_MEM_HOST, should_preprocess, color_correction, chunks, good_mask, CIMBAR_HIP_MEM_HOST, nullptr);
}

// ---- one frame per call, several in flight ------------------------------------------------------------------------------------------
namespace {
constexpr size_t FRAME_OUT_STRIDE = ((size_t)FRAME_BYTES + 15) / 16 * 16;

// the frame in `fs` is complete: its chunks and mask reach the caller's buffers, its return value is parked under its ticket
int frame_slot_finish(cimbar_hip_ctx* ctx, cimbar_hip_ctx::FrameSlot& fs)
{
	if (fs.ticket < 0) return 0;
	const long long ticket = fs.ticket;
	fs.ticket = -1;
	const hipError_t e = hipEventSynchronize(fs.done);
	int rc;
	if (e != hipSuccess) { ctx->err = std::string("decode_frame_wait: ") + hipGetErrorString(e); rc = CIMBAR_HIP_EHIP; }
	else {
		uint32_t mask;
		std::memcpy(&mask, fs.h_out + FRAME_OUT_STRIDE, sizeof mask);
		std::memcpy(fs.user_chunks, fs.h_out, FRAME_BYTES);
		*fs.user_mask = mask;
		rc = CHUNK * __builtin_popcount(mask & ((1u << CHUNKS) - 1u));      // aligned_stream::tellp(): what Decoder::decode_fountain returns (Decoder.h:116-117)
	}
	ctx->fresult[ticket % 16] = {ticket, rc};
	return rc;
}

bool is_page_locked(const void* p)
{
	hipPointerAttribute_t a;
	if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // (memory HIP has never heard of)
	return a.type == hipMemoryTypeHost;
}
}  // namespace

long long cimbar_hip_decode_frame_async(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, size_t stride,
                                        int should_preprocess, int color_correction, uint8_t* chunks, uint32_t* good_mask)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (!rgb || !chunks || !good_mask) { ctx->err = "decode_frame_async: null buffer"; return CIMBAR_HIP_EINVAL; }
	if (stride != 0 && stride < (size_t)width * 3) { ctx->err = "decode_frame_async: stride < width*3"; return CIMBAR_HIP_EINVAL; }
	HIPCHK(hipSetDevice(ctx->device));
	if (width != (unsigned)IMG_W || height != (unsigned)IMG_H || ctx->flood_verify || ctx->timing) {
		// images of another size (CimbReader's padded / too-small cases) and the debugging modes take the one-at-a-time call, behind everything
		// in flight; the result is complete when this returns and is parked under a ticket like any other
		for (auto& fs : ctx->fslot) (void)frame_slot_finish(ctx, fs);
		const long long ticket = ctx->frame_tickets;
		const int rc = cimbar_hip_decode_frame_sync(ctx, rgb, width, height, stride, should_preprocess, color_correction, chunks, good_mask);
		ctx->frame_tickets = ticket + 1;
		ctx->fresult[ticket % 16] = {ticket, rc};
		return ticket;
	}
	rotate_scratch_sets(ctx);
	const int set = ctx->pipe_set;
	cimbar_hip_ctx::FrameSlot& fs = ctx->fslot[set];
	hipStream_t own = ctx->pstream[set];
	(void)frame_slot_finish(ctx, fs);          // at most pipe_depth frames in flight: the one that used this slot is delivered now
	HIPCHK(fs.d_rgb.ensure((size_t)FRAME_RGB));
	HIPCHK(fs.d_out.ensure(FRAME_OUT_STRIDE + 16));
	HIPCHK(fs.h_out.ensure(FRAME_OUT_STRIDE + 16));
	HIPCHK(fs.done.create());
	if (int r = ensure_capacity(ctx, 1)) return r;
	const size_t row = (size_t)IMG_W * 3;
	const uint8_t* src = rgb;
	size_t src_stride = stride ? stride : row;
	if ((ctx->frame_stage || src_stride != row) && !is_page_locked(rgb)) {
		// pageable memory: the caller may reuse (or free: cimbar.cpp:132's cv::Mat lives for one loop iteration) the image as soon as this returns.
		// For a DENSE image that is left to the runtime by default -- a 1-D asynchronous copy out of pageable memory returns once the source has been
		// consumed (it stages the pages itself, measured at 80 us per frame). A STRIDED pageable image (a cv::Mat ROI) would go through
		// hipMemcpy2DAsync, which may pin the user's pages and return with the DMA still pending: such an image is always copied to the context's
		// page-locked staging here (141 us per frame on one host thread), as every pageable image is with CIMBAR_HIP_FRAME_STAGE=1. Either way host
		// work that overlaps the previous frames' kernels. (tests/test_gpu_frame_async.py scribbles over such a buffer right after the call.)
		HIPCHK(fs.h_in.ensure((size_t)FRAME_RGB));
		if (src_stride == row) std::memcpy(fs.h_in, rgb, (size_t)FRAME_RGB);
		else for (int y = 0; y < IMG_H; ++y) std::memcpy(fs.h_in + (size_t)y * row, rgb + (size_t)y * src_stride, row);
		src = fs.h_in;
		src_stride = row;
	}
	hipStream_t cs = own;
	if (ctx->frame_copystream) {
		HIPCHK(ctx->fcopy.create());
		for (Event& e : ctx->ev_fcopy) HIPCHK(e.create());
		cs = ctx->fcopy;
	}
	if (src_stride == row) HIPCHK(hipMemcpyAsync(fs.d_rgb, src, (size_t)FRAME_RGB, hipMemcpyHostToDevice, cs));
	else HIPCHK(hipMemcpy2DAsync(fs.d_rgb, row, src, src_stride, row, (size_t)IMG_H, hipMemcpyHostToDevice, cs));
	if (cs != own) { HIPCHK(hipEventRecord(ctx->ev_fcopy[set], cs)); HIPCHK(hipStreamWaitEvent(own, ctx->ev_fcopy[set], 0)); }
	// the chunks and the mask are written where the host reads them: page-locked host memory is device-visible, the Reed-Solomon kernels store 7.5 KB
	// into it over the link and no copy back (one more DMA packet with its latency) is queued behind the frame
	uint8_t* const out = ctx->frame_zerocopy ? fs.h_out.get() : fs.d_out.get();
	ChainArgs ca;
	ca.d_rgb = fs.d_rgb; ca.n = 1; ca.pre = should_preprocess; ca.cc = color_correction;
	ca.d_chunks = out; ca.d_masks = reinterpret_cast<uint32_t*>(out + FRAME_OUT_STRIDE);
	ca.pipe = true;
	if (int r = enqueue(ctx, own, ca)) return r;
	if (!ctx->frame_zerocopy) HIPCHK(hipMemcpyAsync(fs.h_out, fs.d_out, FRAME_OUT_STRIDE + sizeof(uint32_t), hipMemcpyDeviceToHost, own));
	HIPCHK(hipEventRecord(fs.done, own));
	fs.user_chunks = chunks;
	fs.user_mask = good_mask;
	fs.ticket = ctx->frame_tickets++;
	return fs.ticket;
}

int cimbar_hip_decode_frame_wait(cimbar_hip_ctx* ctx, long long ticket)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (ticket >= 0) {
		for (auto& fs : ctx->fslot) if (fs.ticket == ticket) return frame_slot_finish(ctx, fs);
		const auto& r = ctx->fresult[ticket % 16];
		if (r.ticket == ticket) return r.rc;
	}
	ctx->err = "decode_frame_wait: no such ticket (never issued, or more than 16 frames ago)";
	return CIMBAR_HIP_EINVAL;
}

int cimbar_hip_decode_frame(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, size_t stride,
                            int should_preprocess, int color_correction, uint8_t* chunks, uint32_t* good_mask)
{
	// the synchronous call is the asynchronous one, waited for: the same copies and kernels, one D2H copy for chunks + mask
	const long long t = cimbar_hip_decode_frame_async(ctx, rgb, width, height, stride, should_preprocess, color_correction, chunks, good_mask);
	if (t < 0) return (int)t;
	return cimbar_hip_decode_frame_wait(ctx, t);
}

// ---- extractor stage -------------------------------------------------------------------------------------------------------------
namespace {

// one call per capture format, the format as a compile-time constant (F::value): every kernel that reads a capture is a template on it
template <class Fn>
void for_capture_format(int fmt, Fn&& fn)
{
	switch (fmt) {
	case FMT_RGBA: fn(std::integral_constant<int, FMT_RGBA>{}); break;
	case FMT_NV12: fn(std::integral_constant<int, FMT_NV12>{}); break;
	case FMT_I420: fn(std::integral_constant<int, FMT_I420>{}); break;
	case FMT_NV21: fn(std::integral_constant<int, FMT_NV21>{}); break;
	case FMT_YUYV: fn(std::integral_constant<int, FMT_YUYV>{}); break;
	case FMT_UYVY: fn(std::integral_constant<int, FMT_UYVY>{}); break;
	case FMT_BGR: fn(std::integral_constant<int, FMT_BGR>{}); break;
	case FMT_BGRA: fn(std::integral_constant<int, FMT_BGRA>{}); break;
	default: fn(std::integral_constant<int, FMT_RGB>{}); break;
	}
}
// X1 for n captures: the streaming kernel where the rows can be loaded and stored as aligned 16-byte pieces, else the tiled one
template <int FMT>
void launch_gray_blur_rows(hipStream_t st, unsigned unit, const dim3& g, const uint8_t* d_in, unsigned width, unsigned height, int lanes_out, uint8_t* d_out, uint32_t* d_hist)
{
	if (unit == 3) hipLaunchKernelGGL((k_scan_gray_blur_rows<1, FMT>), g, dim3(256), 0, st, d_in, (int)width, (int)height, lanes_out, d_out, d_hist);
	else hipLaunchKernelGGL((k_scan_gray_blur_rows<2, FMT>), g, dim3(256), 0, st, d_in, (int)width, (int)height, lanes_out, d_out, d_hist);
}
template <bool RGB3>
void launch_gray_blur_tiled(hipStream_t st, unsigned unit, const dim3& g, const uint8_t* d_in, unsigned width, unsigned height, int fmt, uint8_t* d_out, uint32_t* d_hist)
{
	if (unit == 3) hipLaunchKernelGGL((k_scan_gray_blur<1, RGB3>), g, dim3(256), 0, st, d_in, (int)width, (int)height, fmt, d_out, d_hist);
	else if (unit == 5) hipLaunchKernelGGL((k_scan_gray_blur<2, RGB3>), g, dim3(256), 0, st, d_in, (int)width, (int)height, fmt, d_out, d_hist);
	else if (unit == 17) hipLaunchKernelGGL((k_scan_gray_blur<8, RGB3>), g, dim3(256), 0, st, d_in, (int)width, (int)height, fmt, d_out, d_hist);
	else hipLaunchKernelGGL((k_scan_gray_blur<4, RGB3>), g, dim3(256), 0, st, d_in, (int)width, (int)height, fmt, d_out, d_hist);   // 9x9: captures of 2500 px and up
}
void launch_gray_blur(hipStream_t st, unsigned unit, int fmt, const uint8_t* d_in, unsigned width, unsigned height, int n, uint8_t* d_out, uint32_t* d_hist)
{
	static const bool force_tiled = [] { const char* v = std::getenv("CIMBAR_HIP_X1_TILED"); return v && std::atoi(v) != 0; }();
	if (!force_tiled && unit <= 5 && width % 16 == 0 && ((uintptr_t)d_in & 15) == 0 && ((uintptr_t)d_out & 15) == 0) {
		const int groups = (int)width / 16, nb = (groups + 61) / 62, lanes_out = (groups + nb - 1) / nb;   // <= 62 column groups per wavefront + 2 halo lanes
		const int strips = ((int)height + X1S_ROWS - 1) / X1S_ROWS;
		const dim3 g(nb, (strips + 3) / 4, n);
		for_capture_format(fmt, [&](auto F) { launch_gray_blur_rows<decltype(F)::value>(st, unit, g, d_in, width, height, lanes_out, d_out, d_hist); });
		return;
	}
	const dim3 g((width + X1_TW - 1) / X1_TW, (height + X1_TH * X1_TILES - 1) / (X1_TH * X1_TILES), n);
	if (fmt == FMT_RGB) launch_gray_blur_tiled<true>(st, unit, g, d_in, width, height, fmt, d_out, d_hist);
	else launch_gray_blur_tiled<false>(st, unit, g, d_in, width, height, fmt, d_out, d_hist);
}

// X4 for n captures in `fmt`
void launch_warp(hipStream_t st, int fmt, const uint8_t* d_in, unsigned width, unsigned height, int n, const double* d_minv, uint8_t* d_out)
{
	static const int xcd_order = [] { const char* v = std::getenv("CIMBAR_HIP_WARP_ORDER"); return v ? std::atoi(v) : 1; }();
	const dim3 g((IMG_W + 63) / 64, (IMG_H + 16 * WARP_ROWS - 1) / (16 * WARP_ROWS), n);
	for_capture_format(fmt, [&](auto F) { hipLaunchKernelGGL((k_warp<decltype(F)::value>), g, dim3(256), 0, st, d_in, (int)width, (int)height, d_minv, d_out, IMG_W, IMG_H, xcd_order); });
}

// X4 for a context: YUV captures (4:2:0: 12 / 21 / 420; 4:2:2: 422 / 4221) go through k_convert_roi + k_warp<3> (WARP_CHUNK captures at a time through
// one capture-shaped scratch), everything else -- and everything with CIMBAR_HIP_WARP_TWOPASS=0 -- through the warp kernel of its own format.
// (4:2:2 as well: per 256 1080p YUYV captures the extract call takes 2.20 ms this way and 2.44 ms with the conversion inside the warp, the same ratio
// as NV12's -- tools/capture_formats_bench.py, profiles/capture_formats_bench.json)
constexpr int WARP_CHUNK = 512;
int launch_warp_ctx(cimbar_hip_ctx* ctx, hipStream_t st, int fmt, const uint8_t* d_in, unsigned width, unsigned height, int n, const double* d_minv, uint8_t* d_out)
{
	if (!ctx->warp_twopass || !(fmt_is_420(fmt) || fmt_is_422(fmt))) { launch_warp(st, fmt, d_in, width, height, n, d_minv, d_out); return 0; }
	const size_t per = (size_t)width * height * 3, cbytes = capture_bytes(width, height, fmt);
	// captures per pass: WARP_CHUNK, fewer where that many converted captures would not fit the scratch allowance (4 GiB: 512 x 1080p = 3.2 GB; 4K captures go 171 at a time)
	const size_t fit = ctx->warp_scratch / per;
	const int chunk = (int)(fit < 1 ? 1 : (fit < (size_t)WARP_CHUNK ? fit : (size_t)WARP_CHUNK));
	const size_t need = per * (size_t)(n < chunk ? n : chunk);
	if (need > ctx->d_ex_rgb.capacity() || (size_t)n > ctx->d_ex_box.capacity()) HIPCHK(hipStreamSynchronize(st));   // (the scratch a warp still in flight reads is about to be replaced)
	HIPCHK(ctx->d_ex_rgb.reserve(need));
	HIPCHK(ctx->d_ex_box.reserve((size_t)n));
	hipLaunchKernelGGL(k_roi_boxes, dim3((n + 63) / 64), dim3(64), 0, st, d_minv, n, (int)width, (int)height, IMG_W, IMG_H, ctx->d_ex_box);
	for (int lo = 0; lo < n; lo += chunk) {
		const int m = n - lo < chunk ? n - lo : chunk;
		const dim3 gc((width + 127) / 128, (height + 31) / 32, m);
		auto convert = [&](auto F) { hipLaunchKernelGGL((k_convert_roi<decltype(F)::value>), gc, dim3(256), 0, st, d_in + (size_t)lo * cbytes, (int)width, (int)height, ctx->d_ex_box + lo, ctx->d_ex_rgb); };
		switch (fmt) {
		case FMT_NV12: convert(std::integral_constant<int, FMT_NV12>{}); break;
		case FMT_NV21: convert(std::integral_constant<int, FMT_NV21>{}); break;
		case FMT_YUYV: convert(std::integral_constant<int, FMT_YUYV>{}); break;
		case FMT_UYVY: convert(std::integral_constant<int, FMT_UYVY>{}); break;
		default: convert(std::integral_constant<int, FMT_I420>{}); break;
		}
		launch_warp(st, FMT_RGB, ctx->d_ex_rgb, width, height, m, d_minv + (size_t)lo * 9, d_out + (size_t)lo * FRAME_RGB);
	}
	return 0;
}

// the `format` argument as the reference reads it: <= 0 is 3 (cimbar_recv_js.cpp:150-151), 4 / 12 / 420 are get_rgb's cases, everything else its
// default (RGB8) -- but for the five values of native receivers (21 / 422 / 4221 / 30 / 40, extract.hip.inc). The 4:2:0 layouts cannot hold an odd
// width or height, the 4:2:2 ones no odd width (cv::cvtColor asserts; the reference would throw): EDIM.
int check_capture(cimbar_hip_ctx* ctx, const char* who, unsigned width, unsigned height, int format, int* fmt, size_t* bytes)
{
	*fmt = capture_format(format);
	if (!capture_dims_ok(width, height, *fmt)) { ctx->err = std::string(who) + CAPTURE_DIMS_MSG; return CIMBAR_HIP_EDIM; }
	*bytes = capture_bytes(width, height, *fmt);
	if ((uint64_t)width * height * 4 >= (1ull << 33) || *bytes >= ((size_t)1 << 31)) { ctx->err = std::string(who) + ": captures of 2 GiB or more are not supported (the kernels address a capture with 32-bit offsets)"; return CIMBAR_HIP_EDIM; }
	return 0;
}

// Scanner's blur unit (Scanner.h:157-159): max(3, nextPowerOfTwo(min(w, h) * 0.002) + 1)
unsigned scan_blur_unit(unsigned width, unsigned height)
{
	unsigned unit = (unsigned)((width < height ? width : height) * 0.002);
	unit--; unit |= unit >> 1; unit |= unit >> 2; unit |= unit >> 4; unit |= unit >> 8; unit |= unit >> 16;
	return unit + 2 > 3u ? unit + 2 : 3u;
}

int extract_state(cimbar_hip_ctx* ctx, int n)
{
	HIPCHK(ctx->d_ex_hist.reserve((size_t)n * 256));
	HIPCHK(ctx->d_ex_thr.reserve((size_t)n));
	HIPCHK(ctx->d_ex_minv.reserve((size_t)n * 9));
	HIPCHK(ctx->d_scan_hits.reserve((size_t)n * SCAN_MAX_ROWS * SCAN_ROW_PTS));
	HIPCHK(ctx->d_scan_nhits.reserve((size_t)n * SCAN_MAX_ROWS));
	HIPCHK(ctx->d_scan_res.reserve((size_t)n));
	HIPCHK(ctx->d_scan_offs.reserve((size_t)n * (SCAN_MAX_ROWS + 1)));
	HIPCHK(ctx->d_scan_ovf.reserve((size_t)n + 1));           // + the slow path's slot counter
	HIPCHK(ctx->d_scan_serial.ensure((size_t)SCAN_SERIAL_SLOTS * 6 * SCAN_SERIAL_CAP));
	HIPCHK(ctx->d_scan_conf.reserve((size_t)n * SCAN_HMAX));
	HIPCHK(ctx->d_scan_stage.reserve((size_t)n * 2));
	HIPCHK(ctx->h_ex_minv.reserve((size_t)n * 9));
	HIPCHK(ctx->ev_ex_minv.create());
	return 0;
}

}  // namespace

int cimbar_hip_scan_preprocess_fmt(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int format, int n, int rgb_mem,
                                   uint8_t* binary, int* thresholds, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (!rgb || !binary || n <= 0 || width < 8 || height < 8) { ctx->err = "scan_preprocess: null buffer, n <= 0 or a frame smaller than 8x8"; return CIMBAR_HIP_EINVAL; }
	hipStream_t st;
	if (int r = begin_call(ctx, "scan_preprocess", "rgb_mem", rgb_mem, "out_mem", out_mem, hip_stream, &st)) return r;
	const unsigned unit = scan_blur_unit(width, height);
	if (unit != 3 && unit != 5 && unit != 9 && unit != 17) { ctx->err = "scan_preprocess: captures of 8500 px or more on the short side need a 33x33 blur, not implemented"; return CIMBAR_HIP_EDIM; }
	int fmt; size_t cbytes;
	if (int r = check_capture(ctx, "scan_preprocess", width, height, format, &fmt, &cbytes)) return r;
	if (int r = extract_state(ctx, n)) return r;
	const size_t px = (size_t)width * height;
	const uint8_t* d_in = nullptr;
	if (int r = stage_input(ctx, st, ctx->d_ex_in, rgb, cbytes * n, rgb_mem, &d_in)) return r;
	uint8_t* d_out = nullptr;
	if (int r = stage_output(ctx, ctx->d_ex_out, binary, px * n, out_mem, &d_out)) return r;
	HIPCHK(hipMemsetAsync(ctx->d_ex_hist, 0, sizeof(uint32_t) * 256 * (size_t)n, st));
	launch_gray_blur(st, unit, fmt, d_in, width, height, n, d_out, ctx->d_ex_hist);
	hipLaunchKernelGGL(k_scan_otsu, dim3((n + 63) / 64), dim3(64), 0, st, ctx->d_ex_hist, (int)width, (int)height, n, ctx->d_ex_thr);
	hipLaunchKernelGGL(k_scan_binarize, dim3((unsigned)((px + 4095) / 4096), n), dim3(256), 0, st, d_out, px, ctx->d_ex_thr);
	HIPCHK(hipGetLastError());
	if (thresholds) HIPCHK(hipMemcpyAsync(thresholds, ctx->d_ex_thr, sizeof(int) * (size_t)n, out_mem == CIMBAR_HIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
	if (out_mem == CIMBAR_HIP_MEM_DEVICE) return 0;
	HIPCHK(hipMemcpyAsync(binary, d_out, px * n, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return 0;
}

int cimbar_hip_scan_preprocess(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int n, int rgb_mem,
                               uint8_t* binary, int* thresholds, int out_mem, void* hip_stream)
{
	return cimbar_hip_scan_preprocess_fmt(ctx, rgb, width, height, FMT_RGB, n, rgb_mem, binary, thresholds, out_mem, hip_stream);
}

int cimbar_hip_deskew_batch_fmt(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int format, int n, int rgb_mem,
                                const float* corners, uint8_t* frames, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (!rgb || !corners || !frames || n <= 0 || width < 2 || height < 2) { ctx->err = "deskew_batch: null buffer, n <= 0 or an empty frame"; return CIMBAR_HIP_EINVAL; }
	hipStream_t st;
	if (int r = begin_call(ctx, "deskew_batch", "rgb_mem", rgb_mem, "out_mem", out_mem, hip_stream, &st)) return r;
	int fmt; size_t cbytes;
	if (int r = check_capture(ctx, "deskew_batch", width, height, format, &fmt, &cbytes)) return r;
	if (int r = extract_state(ctx, n)) return r;
	// the matrices go through a context-owned pinned buffer: wait for the previous call's copy out of it (long done in practice)
	HIPCHK(hipEventSynchronize(ctx->ev_ex_minv));
	for (int f = 0; f < n; ++f) deskew_inverse_matrix(corners + (size_t)f * 8, ctx->h_ex_minv + (size_t)f * 9);
	HIPCHK(hipMemcpyAsync(ctx->d_ex_minv, ctx->h_ex_minv, sizeof(double) * 9 * (size_t)n, hipMemcpyHostToDevice, st));
	HIPCHK(hipEventRecord(ctx->ev_ex_minv, st));
	const uint8_t* d_in = nullptr;
	if (int r = stage_input(ctx, st, ctx->d_ex_in, rgb, cbytes * n, rgb_mem, &d_in)) return r;
	uint8_t* d_out = nullptr;
	if (int r = stage_output(ctx, ctx->d_ex_out, frames, (size_t)n * FRAME_RGB, out_mem, &d_out)) return r;
	if (int r = launch_warp_ctx(ctx, st, fmt, d_in, width, height, n, ctx->d_ex_minv, d_out)) return r;
	HIPCHK(hipGetLastError());
	if (out_mem == CIMBAR_HIP_MEM_DEVICE) return 0;
	HIPCHK(hipMemcpyAsync(frames, d_out, (size_t)n * FRAME_RGB, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return 0;
}

int cimbar_hip_deskew_batch(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int n, int rgb_mem,
                            const float* corners, uint8_t* frames, int out_mem, void* hip_stream)
{
	return cimbar_hip_deskew_batch_fmt(ctx, rgb, width, height, FMT_RGB, n, rgb_mem, corners, frames, out_mem, hip_stream);
}

namespace {

// X1 + X2 + S1 + S2 + S3 for n device-resident captures: blurred gray -> Otsu -> anchors -> corners / status -> warp matrices.
// Leaves ScanResult[n] in ctx->d_scan_res and the matrices in ctx->d_ex_minv.
int enqueue_scan(cimbar_hip_ctx* ctx, hipStream_t st, const uint8_t* d_in, unsigned width, unsigned height, int fmt, int n)
{
	const unsigned unit = scan_blur_unit(width, height);
	if (unit != 3 && unit != 5 && unit != 9 && unit != 17) { ctx->err = "extract: captures of 8500 px or more on the short side need a 33x33 blur, not implemented"; return CIMBAR_HIP_EDIM; }
	if (width > 65535u || height > 65535u) { ctx->err = "extract: capture larger than 65535 px on a side"; return CIMBAR_HIP_EDIM; }
	const size_t px = (size_t)width * height;
	HIPCHK(ctx->d_ex_gray.reserve(px * n));
	HIPCHK(hipMemsetAsync(ctx->d_ex_hist, 0, sizeof(uint32_t) * 256 * (size_t)n, st));
	launch_gray_blur(st, unit, fmt, d_in, width, height, n, ctx->d_ex_gray, ctx->d_ex_hist);
	hipLaunchKernelGGL(k_scan_otsu, dim3((n + 63) / 64), dim3(64), 0, st, ctx->d_ex_hist, (int)width, (int)height, n, ctx->d_ex_thr);
	// the anchor search (Scanner::scan): primary row scan -> every hit's confirm scans at once -> ordered replay per capture; the same three
	// steps again for the smaller bottom-right anchor in the window the first three predict
	const uint8_t* gimg = ctx->d_ex_gray;
	const int W = (int)width, H = (int)height;
	ScanStage* stage1 = ctx->d_scan_stage;
	ScanStage* stage2 = ctx->d_scan_stage + n;
	const dim3 rows_grid((unsigned)(((size_t)n * SCAN_MAX_ROWS + 3) / 4)), hit_grid(SCAN_HMAX / 4, n);
	hipLaunchKernelGGL(k_scan_stage1, dim3((n + 63) / 64), dim3(64), 0, st, W, H, n, stage1, ctx->d_scan_ovf);
	hipLaunchKernelGGL((k_scan_stage_rows<114>), rows_grid, dim3(256), 0, st, gimg, W, H, ctx->d_ex_thr, stage1, n, ctx->d_scan_hits, ctx->d_scan_nhits);
	hipLaunchKernelGGL(k_scan_offsets, dim3(n), dim3(64), 0, st, ctx->d_scan_nhits, SCAN_MAX_ROWS, SCAN_ROW_PTS, ctx->d_scan_offs, ctx->d_scan_ovf);
	hipLaunchKernelGGL((k_scan_confirm<114>), hit_grid, dim3(256), 0, st, gimg, W, H, ctx->d_ex_thr, ctx->d_scan_hits, ctx->d_scan_offs, stage1, SCAN_MAX_ROWS,
	                   SCAN_ROW_PTS, true, ctx->d_scan_conf, ctx->d_scan_ovf);
	hipLaunchKernelGGL(k_scan_select, dim3(n), dim3(64), 0, st, ctx->d_scan_hits, ctx->d_scan_offs, ctx->d_scan_conf, stage1, W, H, stage2, ctx->d_scan_ovf);
	hipLaunchKernelGGL((k_scan_stage_rows<122>), rows_grid, dim3(256), 0, st, gimg, W, H, ctx->d_ex_thr, stage2, n, ctx->d_scan_hits, ctx->d_scan_nhits);
	hipLaunchKernelGGL(k_scan_offsets, dim3(n), dim3(64), 0, st, ctx->d_scan_nhits, SCAN_MAX_ROWS, SCAN_ROW_PTS, ctx->d_scan_offs, ctx->d_scan_ovf);
	hipLaunchKernelGGL((k_scan_confirm<122>), hit_grid, dim3(256), 0, st, gimg, W, H, ctx->d_ex_thr, ctx->d_scan_hits, ctx->d_scan_offs, stage2, SCAN_MAX_ROWS,
	                   SCAN_ROW_PTS, false, ctx->d_scan_conf, ctx->d_scan_ovf);
	hipLaunchKernelGGL(k_scan_final, dim3(n), dim3(64), 0, st, ctx->d_scan_hits, ctx->d_scan_offs, ctx->d_scan_conf, stage2, W, ctx->d_scan_ovf, ctx->d_scan_res);
	// captures whose search overflowed one of the fixed-size lists above (status -1): Scanner::scan again, serially, lists in global memory
	hipLaunchKernelGGL(k_scan_serial, dim3(n), dim3(64), 0, st, gimg, W, H, ctx->d_ex_thr, ctx->d_scan_serial, ctx->d_scan_ovf + n, ctx->d_scan_ovf, ctx->d_scan_res);
	hipLaunchKernelGGL(k_warp_matrices, dim3((n + 63) / 64), dim3(64), 0, st, ctx->d_scan_res[0].corners, sizeof(ScanResult) / sizeof(float),
	                   &ctx->d_scan_res[0].status, sizeof(ScanResult) / sizeof(int), n, ctx->d_ex_minv);
	HIPCHK(hipGetLastError());
	ctx->scan_n = n;
	ctx->scan_w = width;
	ctx->scan_h = height;
	return 0;
}

// The capture front end: n captures (host memory: staged through d_ex_in) searched -- `scan(d_in)` leaves ScanResult[n] in d_scan_res and the
// warp matrices in d_ex_minv -- and warped into d_out (nullptr: d_ex_frames); `status` (may be nullptr) gets the strided copy of the status words.
template <class Scan>
int capture_front(cimbar_hip_ctx* ctx, hipStream_t st, const uint8_t* img, unsigned width, unsigned height, int fmt, size_t cbytes, int n, int img_mem,
                  uint8_t* d_out, int* status, int out_mem, Scan&& scan)
{
	if (int r = extract_state(ctx, n)) return r;
	const uint8_t* d_in = nullptr;
	if (int r = stage_input(ctx, st, ctx->d_ex_in, img, cbytes * n, img_mem, &d_in)) return r;
	if (!d_out) { HIPCHK(ctx->d_ex_frames.reserve((size_t)n * FRAME_RGB)); d_out = ctx->d_ex_frames; }
	if (int r = scan(d_in)) return r;
	if (int r = launch_warp_ctx(ctx, st, fmt, d_in, width, height, n, ctx->d_ex_minv, d_out)) return r;
	HIPCHK(hipGetLastError());
	const hipMemcpyKind kind = out_mem == CIMBAR_HIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
	if (status) HIPCHK(hipMemcpy2DAsync(status, sizeof(int), &ctx->d_scan_res[0].status, sizeof(ScanResult), sizeof(int), (size_t)n, kind, st));
	return 0;
}
// ... with the anchor search itself (X1 + X2 + S1-S3, enqueue_scan)
int capture_front(cimbar_hip_ctx* ctx, hipStream_t st, const uint8_t* img, unsigned width, unsigned height, int fmt, size_t cbytes, int n, int img_mem,
                  uint8_t* d_out, int* status, int out_mem)
{
	return capture_front(ctx, st, img, width, height, fmt, cbytes, n, img_mem, d_out, status, out_mem,
	                     [&](const uint8_t* d_in) { return enqueue_scan(ctx, st, d_in, width, height, fmt, n); });
}

// what a decode tail reads: n device-resident frames and what came with them
struct FrameSource {
	const uint8_t* d_frames = nullptr;
	const int* d_status = nullptr; int stride = 0;   // the extraction status per frame, `stride` ints apart (nullptr: frame input, every frame usable)
	int pre = 0; bool guess = false;                 // sharpen every frame / where the extractor said NEEDS_SHARPEN (d_status)
	bool captures = false;                           // deskewed captures: one chain (ChainArgs::no_split), and what the extractor gave up on is masked
	PadSource pad{};
};

// the caller's frames (host memory: staged through d_rgb)
int frames_source(cimbar_hip_ctx* ctx, hipStream_t st, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, FrameSource* fs)
{
	fs->pre = should_preprocess;
	return stage_input(ctx, st, ctx->d_rgb, rgb, (size_t)n * FRAME_RGB, rgb_mem, &fs->d_frames);
}

// the frames a capture front end left in d_ex_frames, with their status words. cimbar.cpp:131,147-154: preprocess 1 = sharpen every frame,
// 0 = none, anything else = where the extractor said NEEDS_SHARPEN
FrameSource deskewed_source(cimbar_hip_ctx* ctx, const int* d_status, int stride, int preprocess)
{
	FrameSource fs;
	fs.d_frames = ctx->d_ex_frames; fs.d_status = d_status; fs.stride = stride;
	fs.pre = preprocess == 1 ? 1 : 0; fs.guess = preprocess != 0 && preprocess != 1;
	fs.captures = true;
	return fs;
}

// the caller's captures through the front end (extraction runs for every capture: the once-calls find their runs on the deskewed frames)
int captures_source(cimbar_hip_ctx* ctx, hipStream_t st, const CaptureIn& cap, const uint8_t* img, int n, int img_mem, int preprocess, int out_mem, FrameSource* fs)
{
	if (int r = capture_front(ctx, st, img, cap.width, cap.height, cap.fmt, cap.cbytes, n, img_mem, nullptr, cap.status, out_mem)) return r;
	*fs = deskewed_source(ctx, &ctx->d_scan_res[0].status, (int)(sizeof(ScanResult) / sizeof(int)), preprocess);
	return 0;
}

// enqueue()'s arguments for n frames of a source
ChainArgs chain_args(const FrameSource& fs, int n, int cc, uint8_t* d_chunks, uint32_t* d_masks)
{
	ChainArgs ca;
	ca.d_rgb = fs.d_frames; ca.n = n; ca.pre = fs.pre; ca.cc = cc;
	ca.d_chunks = d_chunks; ca.d_masks = d_masks;
	if (fs.guess) { ca.d_sel = fs.d_status; ca.sel_stride = fs.stride; }
	ca.no_split = fs.captures;
	ca.pad = fs.pad;
	return ca;
}

// the decode chain over a source and, behind it and in front of any combine / stitch, the masking of the captures the extractor gave up on:
// the reference skips them (cimbar.cpp:141-146), nothing of them reaches the sink, a group or a stitched pair
int enqueue_source(cimbar_hip_ctx* ctx, hipStream_t st, const FrameSource& fs, int n, int cc, uint8_t* d_chunks, uint32_t* d_masks)
{
	if (int r = enqueue(ctx, st, chain_args(fs, n, cc, d_chunks, d_masks))) return r;
	if (fs.captures) {
		hipLaunchKernelGGL(k_mask_failed, dim3(n), dim3(256), 0, st, fs.d_status, fs.stride, n, d_masks, d_chunks);
		HIPCHK(hipGetLastError());
	}
	return 0;
}

// "decode_batch" + tail for frames, "scan_extract_decode_batch" + tail for captures: what the messages call an entry point
std::string call_name(const CaptureIn* cap, const char* tail) { return std::string(cap ? "scan_extract_decode_batch" : "decode_batch") + tail; }

// What the decode entry points check of their input, in this order: null buffers / n (captures: / 8x8), then the call prologue with its mem
// flags (begin_call), then -- captures -- what the format can hold (EDIM; cap->fmt and cap->cbytes are resolved here). `flush`: a
// combined-stream call with n == 0, which reads no image argument.
int begin_decode(cimbar_hip_ctx* ctx, const char* who, CaptureIn* cap, const void* img, int n, const char* in_name, int img_mem, bool outputs, int out_mem,
                 void* hip_stream, bool flush, hipStream_t* st)
{
	if (!flush && (!img || !outputs || n <= 0 || (cap && (cap->width < 8 || cap->height < 8)))) {
		ctx->err = std::string(who) + (cap ? ": null buffer, n <= 0 or a capture smaller than 8x8" : ": null buffer or n <= 0");
		return CIMBAR_HIP_EINVAL;
	}
	// (a quirk, kept: the flush of the capture call checks out_mem alone and accepts any img_mem; that of the frame call checks both flags)
	if (int r = begin_call(ctx, who, (flush && cap) ? nullptr : in_name, img_mem, "out_mem", out_mem, hip_stream, st)) return r;
	if (cap && !flush) return check_capture(ctx, who, cap->width, cap->height, cap->format, &cap->fmt, &cap->cbytes);
	return 0;
}

int64_t decode_impl(cimbar_hip_ctx* ctx, CaptureIn* cap, const uint8_t* img, int n, int img_mem, int preprocess, int color_correction, uint8_t* chunks,
                    uint32_t* masks, int out_mem, void* hip_stream, CombineArgs* cb, StitchArgs* sa, const PadSource* pad)
{
	const bool strm = cb && cb->stream;
	const std::string name = call_name(cap, sa ? (sa->stream ? "_stitched_stream" : "_stitched") : strm ? "_combined_stream" : cb ? "_combined" : "");
	const char* who = name.c_str();
	// (a stream call may bring no capture at all: n == 0 with a flush closes the open group)
	const bool flush = strm && n == 0;
	hipStream_t st;
	if (int r = begin_decode(ctx, who, cap, img, n, "rgb_mem", img_mem, chunks && masks, out_mem, hip_stream, flush, &st)) return r;
	if (cb) if (int r = check_combine(ctx, who, n, *cb)) return r;
	if (sa) if (int r = check_stitch(ctx, who, n, *sa)) return r;
	if (flush) {
		if (int r = enqueue_combine_stream(ctx, st, 0, nullptr, nullptr, nullptr, nullptr, 0, *cb, out_mem)) return r;
		return finish_stream(ctx, st, 0, chunks, masks, nullptr, nullptr, out_mem, *cb);
	}
	// (a stitched-stream call waits for the one before in front of every reservation and staging copy)
	if (sa && sa->stream) if (int r = begin_stitch_stream(ctx, st)) return r;
	if (int r = ensure_capacity(ctx, n)) return r;
	FrameSource fs;
	if (int r = cap ? captures_source(ctx, st, *cap, img, n, img_mem, preprocess, out_mem, &fs) : frames_source(ctx, st, img, n, img_mem, preprocess, &fs)) return r;
	if (pad) fs.pad = *pad;
	uint8_t* d_chunks = out_mem == CIMBAR_HIP_MEM_DEVICE ? chunks : ctx->d_chunks;
	uint32_t* d_masks = out_mem == CIMBAR_HIP_MEM_DEVICE ? masks : ctx->d_masks;
	if (int r = enqueue_source(ctx, st, fs, n, color_correction, d_chunks, d_masks)) return r;
	if (strm) {
		if (int r = enqueue_combine_stream(ctx, st, n, fs.d_frames, d_chunks, d_masks, fs.d_status, fs.stride, *cb, out_mem)) return r;
		return finish_stream(ctx, st, n, chunks, masks, d_chunks, d_masks, out_mem, *cb);
	}
	if (cb) if (int r = enqueue_combine(ctx, st, n, fs.d_frames, d_chunks, d_masks, fs.d_status, fs.stride, *cb, out_mem)) return r;
	if (sa && sa->rows(n) > 0) if (int r = enqueue_stitch(ctx, st, n, fs.d_frames, fs.d_status, fs.stride, *sa, out_mem)) return r;
	const int64_t rc = sa ? finish_stitched(ctx, st, n, chunks, masks, d_chunks, d_masks, out_mem, *sa) : finish_batch(ctx, st, n, chunks, masks, d_chunks, d_masks, out_mem, cb);
	// (host outputs of a plain or stitched call: it has synchronised, so the stage timers of its chain can be read)
	if (rc >= 0 && !cb && out_mem == CIMBAR_HIP_MEM_HOST && ctx->timing) if (int r = read_stage_times(ctx)) return r;
	return rc;
}

}  // namespace

int cimbar_hip_extract_batch_fmt(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int format, int n, int rgb_mem, uint8_t* frames,
                                 int* status, float* corners, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (!rgb || !frames || !status || n <= 0 || width < 8 || height < 8) { ctx->err = "extract_batch: null buffer, n <= 0 or a capture smaller than 8x8"; return CIMBAR_HIP_EINVAL; }
	hipStream_t st;
	if (int r = begin_call(ctx, "extract_batch", "rgb_mem", rgb_mem, "out_mem", out_mem, hip_stream, &st)) return r;
	int fmt; size_t cbytes;
	if (int r = check_capture(ctx, "extract_batch", width, height, format, &fmt, &cbytes)) return r;
	uint8_t* d_out = nullptr;
	if (int r = stage_output(ctx, ctx->d_ex_out, frames, (size_t)n * FRAME_RGB, out_mem, &d_out)) return r;
	if (int r = capture_front(ctx, st, rgb, width, height, fmt, cbytes, n, rgb_mem, d_out, status, out_mem)) return r;
	const hipMemcpyKind kind = out_mem == CIMBAR_HIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
	if (corners) HIPCHK(hipMemcpy2DAsync(corners, sizeof(float) * 8, ctx->d_scan_res[0].corners, sizeof(ScanResult), sizeof(float) * 8, (size_t)n, kind, st));
	if (out_mem == CIMBAR_HIP_MEM_DEVICE) return 0;
	HIPCHK(hipMemcpyAsync(frames, d_out, (size_t)n * FRAME_RGB, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return 0;
}

int cimbar_hip_extract_batch(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int n, int rgb_mem, uint8_t* frames,
                             int* status, float* corners, int out_mem, void* hip_stream)
{
	return cimbar_hip_extract_batch_fmt(ctx, rgb, width, height, FMT_RGB, n, rgb_mem, frames, status, corners, out_mem, hip_stream);
}

int64_t cimbar_hip_scan_extract_decode_batch_fmt(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int format, int n, int rgb_mem,
                                                 int preprocess, int color_correction, uint8_t* chunks, uint32_t* masks, int* status, int out_mem,
                                                 void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	CaptureIn cap{width, height, format, status};
	return decode_impl(ctx, &cap, rgb, n, rgb_mem, preprocess, color_correction, chunks, masks, out_mem, hip_stream, nullptr);
}

int64_t cimbar_hip_scan_extract_decode_batch_combined_fmt(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int format, int n,
                                                          int rgb_mem, int preprocess, int color_correction, const int* groups_in, int min_agree_permille,
                                                          int max_group, uint8_t* chunks, uint32_t* masks, int* status, int* groups_out,
                                                          uint8_t* gchunks, uint32_t* gmasks, int* n_groups, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	CombineArgs cb{groups_in, min_agree_permille, max_group, groups_out, gchunks, gmasks, n_groups};
	CaptureIn cap{width, height, format, status};
	return decode_impl(ctx, &cap, rgb, n, rgb_mem, preprocess, color_correction, chunks, masks, out_mem, hip_stream, &cb);
}

int64_t cimbar_hip_scan_extract_decode_batch_stitched_fmt(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int format, int n,
                                                          int rgb_mem, int preprocess, int color_correction, int axis, int min_agree_permille,
                                                          int min_band, uint8_t* chunks, uint32_t* masks, int* status, uint8_t* schunks,
                                                          uint32_t* smasks, int32_t* tears, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	StitchArgs sa{axis, min_agree_permille, min_band, schunks, smasks, tears, {}};
	CaptureIn cap{width, height, format, status};
	return decode_impl(ctx, &cap, rgb, n, rgb_mem, preprocess, color_correction, chunks, masks, out_mem, hip_stream, nullptr, &sa);
}

int64_t cimbar_hip_scan_extract_decode_batch_stitched_stream_fmt(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int format,
                                                                 int n, int rgb_mem, int preprocess, int color_correction, int axis,
                                                                 int min_agree_permille, int min_band, uint8_t* chunks, uint32_t* masks, int* status,
                                                                 uint8_t* schunks, uint32_t* smasks, int32_t* tears, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	StitchArgs sa{axis, min_agree_permille, min_band, schunks, smasks, tears, {}, true};
	CaptureIn cap{width, height, format, status};
	return decode_impl(ctx, &cap, rgb, n, rgb_mem, preprocess, color_correction, chunks, masks, out_mem, hip_stream, nullptr, &sa);
}

int64_t cimbar_hip_scan_extract_decode_batch_combined_stream_fmt(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int format,
                                                                 int n, int rgb_mem, int preprocess, int color_correction, int min_agree_permille,
                                                                 int max_group, int flush, uint8_t* chunks, uint32_t* masks, int* status,
                                                                 int* groups_out, uint8_t* gchunks, uint32_t* gmasks, int* gsizes, int* n_groups,
                                                                 int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	CombineArgs cb{nullptr, min_agree_permille, max_group, groups_out, gchunks, gmasks, n_groups, true, flush, gsizes};
	CaptureIn cap{width, height, format, status};
	return decode_impl(ctx, &cap, rgb, n, rgb_mem, preprocess, color_correction, chunks, masks, out_mem, hip_stream, &cb);
}

int64_t cimbar_hip_scan_extract_decode_batch(cimbar_hip_ctx* ctx, const uint8_t* rgb, unsigned width, unsigned height, int n, int rgb_mem,
                                             int preprocess, int color_correction, uint8_t* chunks, uint32_t* masks, int* status, int out_mem,
                                             void* hip_stream)
{
	return cimbar_hip_scan_extract_decode_batch_fmt(ctx, rgb, width, height, FMT_RGB, n, rgb_mem, preprocess, color_correction, chunks, masks, status, out_mem, hip_stream);
}

namespace {

// ------------------------------------------------------------------------------------------------ repeat-capture skipping (repeat.hip.inc)
struct OnceArgs {
	int min_agree, max_run;   // resolved by check_once (900 / 4 for <= 0)
	int* runs_out; int* roles; uint8_t* rchunks; uint32_t* rmasks; int* n_runs;   // each may be nullptr
	bool stream = false;      // a once-stream call: run 0 may continue the run the call before left (after begin_once_stream)
	int* continued = nullptr; // ... and whether it does (may be nullptr)
};

// the argument checks of the once entry points, before anything is enqueued
int check_once(cimbar_hip_ctx* ctx, const char* who, OnceArgs& oa)
{
	if (LEGACY) { ctx->err = std::string(who) + ": modes 4 and 8 are not covered; the ink signature was checked on the palettes of modes 68 / 67 / 66"; return CIMBAR_HIP_EINVAL; }
	if (oa.min_agree > 1000) { ctx->err = std::string(who) + ": min_agree_permille above 1000"; return CIMBAR_HIP_EINVAL; }
	if (oa.max_run > GMAX) { ctx->err = std::string(who) + ": max_run above 8"; return CIMBAR_HIP_EINVAL; }
	if (oa.min_agree <= 0) oa.min_agree = RP_AGREE_DEFAULT;
	if (oa.max_run <= 0) oa.max_run = RP_RUN_DEFAULT;
	return 0;
}

// room for the gathered frames of a list of `len` captures and for what their decode delivers
int ensure_once_list(cimbar_hip_ctx* ctx, int len)
{
	HIPCHK(ctx->d_rp_frames.reserve((size_t)len * FRAME_RGB));
	HIPCHK(ctx->d_rp_chunks.reserve((size_t)len * FRAME_BYTES));
	HIPCHK(ctx->d_rp_masks.reserve((size_t)len));
	HIPCHK(ctx->d_rp_sel.reserve((size_t)len));
	return 0;
}

// the run rescue's buffers for a call of n captures and `slots` rescue slots: the store of the representatives' cells, the group scratch
// (the combined calls': a slot is a group slot, d_gchunks / d_gmasks the slot staging) and the small maps
int ensure_rescue_capacity(cimbar_hip_ctx* ctx, int n, int slots)
{
	const size_t S = (size_t)slots;
	if (int r = ensure_group_capacity(ctx, slots)) return r;
	HIPCHK(ctx->d_rs_symbols.reserve(S * CS_CELLS));
	HIPCHK(ctx->d_rs_colors.reserve(S * CS_CELLS));
	HIPCHK(ctx->d_rs_drift.reserve(S * CS_DRIFT));
	HIPCHK(ctx->d_rs_plane.reserve(S * CS_PLANE));
	HIPCHK(ctx->d_rs_flood.reserve(S));
	HIPCHK(ctx->d_rs_run.reserve(S));
	HIPCHK(ctx->d_rs_count.ensure(1));
	HIPCHK(ctx->d_rs_map.reserve((size_t)n));
	HIPCHK(ctx->d_rs_tap.reserve((size_t)n));
	return 0;
}

// the store as the group kernels take it (what a rescue member has no use for stays null: its chunks and mask are the call's own outputs)
CarryStore rescue_store(cimbar_hip_ctx* ctx)
{
	return CarryStore{ctx->d_rs_symbols, ctx->d_rs_colors, ctx->d_rs_plane, ctx->d_rs_drift, ctx->d_rs_flood, nullptr, nullptr, nullptr, nullptr};
}

// the 4-byte count d_words[which] (h_words: its page-locked mirror), read back behind everything enqueued on `st` so far
int once_read_count(cimbar_hip_ctx* ctx, hipStream_t st, const int* d_words, int* h_words, int which, int* out)
{
	HIPCHK(hipMemcpyAsync(h_words + which, d_words + which, sizeof(int), hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	*out = ((volatile int*)h_words)[which];
	return 0;
}

// the start of a once-stream call, behind its argument checks: the carry store (allocated by the first such call, nothing carried) and the
// wait that puts the whole call behind the once-stream call before, whatever their streams
int begin_once_stream(cimbar_hip_ctx* ctx, hipStream_t st)
{
	if (!ctx->ostream) ctx->ostream = std::make_unique<OnceStream>();
	OnceStream& s = *ctx->ostream;
	HIPCHK(s.ev_last.create());
	HIPCHK(s.sig.ensure((size_t)2 * RP_CARRY_SIG));
	HIPCHK(s.row.ensure((size_t)2 * RP_CARRY_ROW));
	HIPCHK(s.cw.ensure(RP_CALL_WORDS));
	HIPCHK(s.h_cw.ensure(RP_CALL_WORDS));
	if (!s.words) { HIPCHK(s.words.ensure((size_t)2 * RP_CARRY_WORDS)); HIPCHK(hipMemset(s.words, 0, sizeof(uint32_t) * 2 * RP_CARRY_WORDS)); }
	if (s.used) HIPCHK(hipStreamWaitEvent(st, s.ev_last, 0));
	return 0;
}

// the end of a once-stream call, failed or not: the event the next one waits for, behind whatever this one enqueued
int64_t end_once_stream(cimbar_hip_ctx* ctx, hipStream_t st, int64_t rc)
{
	OnceStream& s = *ctx->ostream;
	if (hipEventRecord(s.ev_last, st) == hipSuccess) s.used = true;
	else if (rc >= 0) { ctx->err = "once_stream: hipEventRecord failed"; return CIMBAR_HIP_EHIP; }
	return rc;
}

// Everything behind the input: the n device-resident frames of `src` (the caller's, or the warp's, with the capture path's extraction status).
// R1-R5 and G2, the read-back of the run count, pass 1, the read-back of list 2's length, pass 2, R8 and the outputs.
int64_t once_impl(cimbar_hip_ctx* ctx, hipStream_t st, const FrameSource& src, int n, int cc, uint8_t* chunks, uint32_t* masks, const OnceArgs& oa, int out_mem)
{
	const size_t N = (size_t)n;
	const bool dev = out_mem == CIMBAR_HIP_MEM_DEVICE, guess = src.guess;
	const uint8_t* const d_frames = src.d_frames; const int* const d_status = src.d_status; const int stride = src.stride;
	HIPCHK(ctx->d_rp_sums.reserve(N * NCELLS));
	HIPCHK(ctx->d_rp_sig.reserve(N * NCELLS));
	HIPCHK(ctx->d_rp_agree.reserve(N));
	HIPCHK(ctx->d_rp_runs.reserve(N));
	HIPCHK(ctx->d_rp_mem.reserve(N * GMAX));
	HIPCHK(ctx->d_rp_count.reserve(N));
	HIPCHK(ctx->d_rp_roles.reserve(N));
	HIPCHK(ctx->d_rp_list.reserve(2 * N));
	HIPCHK(ctx->d_rp_words.ensure(2));
	HIPCHK(ctx->h_rp_words.ensure(2));
	// host-bound per-capture results go through the staging every batch call uses; it must hold all n slots whatever the passes' sizes
	HIPCHK(ctx->d_chunks.reserve(N * FRAME_BYTES));
	HIPCHK(ctx->d_masks.reserve(N));
	uint8_t* d_chunks = dev ? chunks : ctx->d_chunks.get();
	uint32_t* d_masks = dev ? masks : ctx->d_masks.get();
	ctx->rp_n = 0;
	// a once-stream call: the carry it reads, and its own words (list 1 may be shorter than the run count)
	OnceStream* os = oa.stream ? ctx->ostream.get() : nullptr;
	const RepeatCarry cy = os ? os->carry() : RepeatCarry{};
	int* d_words = os ? os->cw.get() : ctx->d_rp_words.get();
	int* h_words = os ? os->h_cw.get() : ctx->h_rp_words.get();
	const int w_len1 = os ? (int)RPC_LEN1 : 0, w_len2 = os ? (int)RPC_LEN2 : 1;
	// the run rescue (cimbar_hip_set_once_rescue): the plain once-calls only, and only where a run row is asked for
	const bool rescue = ctx->rs_on != 0 && !os && (oa.rchunks || oa.rmasks);
	int rs_slots = 0;
	ctx->rs_state = 0;
	// tear skipping (cimbar_hip_set_once_tear_skip): the plain once-calls only. List 1 is then no longer "one per run": its length and list
	// 2's come from the setting's own words, and pass 1's results are addressed through d_rt_pos.
	const bool tear = ctx->rt_axis >= 0 && !os;
	ctx->rt_state = false;
	// tear salvage (cimbar_hip_set_once_tear_salvage): effective only where the rescue and tear skipping both are
	const bool salvage = ctx->sv_on != 0 && rescue && tear;
	ctx->sv_state = false;
	if (tear) {
		HIPCHK(ctx->d_rt_tap.reserve(N * 4));
		HIPCHK(ctx->d_rt_pos.reserve(N));
		HIPCHK(ctx->d_rt_words.ensure(RT_WORDS));
		HIPCHK(ctx->h_rt_words.ensure(RT_WORDS));
	}

	hipLaunchKernelGGL(k_repeat_sums, dim3(DIM_Y, n), dim3(256), 0, st, d_frames, ctx->tb, ctx->d_rp_sums);
	hipLaunchKernelGGL(k_repeat_sig, dim3(n), dim3(256), 0, st, ctx->d_rp_sums, ctx->d_rp_sig);
	if (os) {
		hipLaunchKernelGGL(k_repeat_agree_stream, dim3(n), dim3(256), 0, st, ctx->d_rp_sig, cy, ctx->d_rp_agree);
		hipLaunchKernelGGL(k_repeat_walk_stream, dim3(1), dim3(64), 0, st, ctx->d_rp_agree, n, d_status, stride, oa.min_agree, oa.max_run, cy, ctx->d_rp_runs,
		                   ctx->d_rp_mem, ctx->d_rp_count, d_words);
		hipLaunchKernelGGL(k_repeat_lists_stream, dim3((n + 255) / 256), dim3(256), 0, st, ctx->d_rp_runs, ctx->d_rp_mem, ctx->d_rp_count, n, d_words, ctx->d_rp_roles,
		                   ctx->d_rp_list);
	} else {
		if (n > 1) hipLaunchKernelGGL(k_repeat_agree, dim3(n - 1), dim3(256), 0, st, ctx->d_rp_sig, n, ctx->d_rp_agree);
		HIPCHK(hipMemsetAsync(ctx->d_rp_count, 0, sizeof(int) * N, st));
		HIPCHK(hipMemsetAsync(ctx->d_rp_words, 0, sizeof(int) * 2, st));
		hipLaunchKernelGGL(k_group_walk, dim3(1), dim3(64), 0, st, ctx->d_rp_agree, n, d_status, stride, (const int*)nullptr, oa.min_agree, oa.max_run,
		                   ctx->d_rp_runs, ctx->d_rp_mem, ctx->d_rp_count, ctx->d_rp_words);
		if (tear) {
			hipLaunchKernelGGL(k_repeat_tear, dim3(n), dim3(256), 0, st, ctx->d_rp_sig, ctx->d_rp_runs, ctx->d_rp_count, n, ctx->tb_stitch_line, ctx->rt_axis, ctx->rt_line,
			                   ctx->rt_side, ctx->d_rt_tap);
			hipLaunchKernelGGL(k_repeat_lists_tear, dim3(1), dim3(64), 0, st, ctx->d_rp_runs, ctx->d_rp_mem, ctx->d_rp_count, n, ctx->d_rt_tap, ctx->d_rp_roles,
			                   ctx->d_rp_list, ctx->d_rt_pos, ctx->d_rt_words);
		} else
			hipLaunchKernelGGL(k_repeat_lists, dim3((n + 255) / 256), dim3(256), 0, st, ctx->d_rp_runs, ctx->d_rp_mem, ctx->d_rp_count, n, ctx->d_rp_roles, ctx->d_rp_list);
	}
	HIPCHK(hipGetLastError());
	int len1 = 0, len2 = 0;
	// (tear skipping: the same read-back, of the length of list 1 -- the run count less the candidates; the run count itself is needed by
	// the device alone until the call's last copy)
	if (tear) { if (int r = once_read_count(ctx, st, ctx->d_rt_words, ctx->h_rt_words, RTW_LEN1, &len1)) return r; }
	else if (int r = once_read_count(ctx, st, d_words, h_words, w_len1, &len1)) return r;
	if (len1 < 0 || len1 > n) { ctx->err = "decode_batch_once: the run count read back is out of range"; return CIMBAR_HIP_EHIP; }

	// one decode pass over `len` listed captures: gather, enqueue() as one plain batch of the entry point's kind, scatter
	auto pass = [&](const int* d_list, int len) -> int {
		if (int r = ensure_once_list(ctx, len)) return r;
		if (int r = ensure_capacity(ctx, len)) return r;
		hipLaunchKernelGGL(k_repeat_gather, dim3(96, len), dim3(256), 0, st, d_frames, d_list, ctx->d_rp_frames, guess ? d_status : (const int*)nullptr, stride, ctx->d_rp_sel);
		FrameSource gathered = src;
		gathered.d_frames = ctx->d_rp_frames; gathered.d_status = ctx->d_rp_sel; gathered.stride = 1;
		if (int r = enqueue(ctx, st, chain_args(gathered, len, cc, ctx->d_rp_chunks, ctx->d_rp_masks))) return r;
		hipLaunchKernelGGL(k_repeat_scatter, dim3(len), dim3(256), 0, st, d_list, ctx->d_rp_chunks, ctx->d_rp_masks, d_chunks, d_masks);
		HIPCHK(hipGetLastError());
		return 0;
	};
	if (len1 == n) {
		// every capture is its own run: pass 1 decodes the input in place, and there is nobody for a pass 2
		if (int r = ensure_capacity(ctx, n)) return r;
		if (int r = enqueue(ctx, st, chain_args(src, n, cc, d_chunks, d_masks))) return r;
	} else {
		hipLaunchKernelGGL(k_repeat_clear, dim3(n), dim3(256), 0, st, ctx->d_rp_roles, d_chunks, d_masks);
		if (len1 > 0) {
			if (int r = pass(ctx->d_rp_list, len1)) return r;
			if (os)
				hipLaunchKernelGGL(k_repeat_lists2_stream, dim3(1), dim3(64), 0, st, ctx->d_rp_runs, ctx->d_rp_masks, n, cy, ctx->d_rp_roles, ctx->d_rp_list + n, d_words);
			else {
				if (rescue) HIPCHK(ctx->d_rs_map.reserve(N));
				if (tear)
					hipLaunchKernelGGL(k_repeat_lists2_tear, dim3(1), dim3(64), 0, st, ctx->d_rp_runs, ctx->d_rp_masks, ctx->d_rt_pos, n, ctx->d_rp_roles, ctx->d_rp_list + n,
					                   ctx->d_rt_words + RTW_LEN2, rescue ? ctx->d_rs_map.get() : (int*)nullptr);
				else
					hipLaunchKernelGGL(k_repeat_lists2, dim3(1), dim3(64), 0, st, ctx->d_rp_runs, ctx->d_rp_masks, n, ctx->d_rp_roles, ctx->d_rp_list + n, ctx->d_rp_words + 1,
					                   rescue ? ctx->d_rs_map.get() : (int*)nullptr);
			}
			HIPCHK(hipGetLastError());
			if (tear) { if (int r = once_read_count(ctx, st, ctx->d_rt_words, ctx->h_rt_words, RTW_LEN2, &len2)) return r; }
			else if (int r = once_read_count(ctx, st, d_words, h_words, w_len2, &len2)) return r;
			if (len2 < 0 || len2 > n - len1) { ctx->err = "decode_batch_once: the fallback count read back is out of range"; return CIMBAR_HIP_EHIP; }
			if (rescue && len2 > 0) {
				// pass 2 overwrites pass 1's scratch: the representatives of the runs that may need the rescue are saved first
				// (tear salvage: a capture of list 2 may be the partial of the runs on both its sides)
				rs_slots = salvage ? (len1 < 2 * len2 ? len1 : 2 * len2) : (len1 < len2 ? len1 : len2);
				if (int r = ensure_rescue_capacity(ctx, n, rs_slots)) return r;
				cimbar_hip_ctx::ScratchSet& p1 = ctx->cur();
				if (salvage) {
					HIPCHK(ctx->d_sv_part.reserve((size_t)rs_slots * 8));
					HIPCHK(ctx->d_sv_full.reserve((size_t)rs_slots));
					hipLaunchKernelGGL(k_rescue_save_salvage, dim3(RS_ARRAYS * RS_PARTS, rs_slots), dim3(256), 0, st, p1.d_plane, p1.d_symbols, p1.d_colors, p1.d_drift,
					                   p1.d_flood, ctx->d_rp_masks, ctx->d_rp_mem, ctx->d_rp_count, n, rescue_store(ctx), ctx->d_rs_run, ctx->d_gmem, ctx->d_rs_map,
					                   ctx->d_rs_count, ctx->d_rt_pos, ctx->d_rp_roles, ctx->d_rt_tap, n, ctx->sv_guard, ctx->d_sv_part);
				} else if (tear)
					hipLaunchKernelGGL(k_rescue_save_tear, dim3(RS_ARRAYS * RS_PARTS, rs_slots), dim3(256), 0, st, p1.d_plane, p1.d_symbols, p1.d_colors, p1.d_drift, p1.d_flood,
					                   ctx->d_rp_masks, ctx->d_rp_mem, ctx->d_rp_count, n, rescue_store(ctx), ctx->d_rs_run, ctx->d_gmem, ctx->d_rs_map, ctx->d_rs_count,
					                   ctx->d_rt_pos);
				else
					hipLaunchKernelGGL(k_rescue_save, dim3(RS_ARRAYS * RS_PARTS, rs_slots), dim3(256), 0, st, p1.d_plane, p1.d_symbols, p1.d_colors, p1.d_drift, p1.d_flood,
					                   ctx->d_rp_masks, ctx->d_rp_mem, ctx->d_rp_count, len1, rescue_store(ctx), ctx->d_rs_run, ctx->d_gmem, ctx->d_rs_map, ctx->d_rs_count);
				HIPCHK(hipGetLastError());
			}
			if (len2 > 0) if (int r = pass(ctx->d_rp_list + n, len2)) return r;
		}
	}
	uint8_t* d_rchunks = oa.rchunks;
	uint32_t* d_rmasks = oa.rmasks;
	if (!dev) {
		if (oa.rchunks) { HIPCHK(ctx->d_rp_rchunks.reserve(N * FRAME_BYTES)); d_rchunks = ctx->d_rp_rchunks; }
		if (oa.rmasks) { HIPCHK(ctx->d_rp_rmasks.reserve(N)); d_rmasks = ctx->d_rp_rmasks; }
	}
	if (os) {
		if (d_rchunks || d_rmasks)
			hipLaunchKernelGGL(k_repeat_end_stream, dim3(n), dim3(256), 0, st, ctx->d_rp_mem, ctx->d_rp_count, d_words, d_chunks, d_masks, cy, d_rchunks, d_rmasks);
		// the call's last kernel: it writes the slot this call does not read, and the slots change roles only where the call returns its result
		hipLaunchKernelGGL(k_repeat_carry, dim3(1), dim3(256), 0, st, ctx->d_rp_sig, ctx->d_rp_runs, ctx->d_rp_mem, ctx->d_rp_count, d_words, d_chunks, d_masks, n, cy);
	} else if (d_rchunks || d_rmasks)
		hipLaunchKernelGGL(k_repeat_end, dim3(n), dim3(256), 0, st, ctx->d_rp_mem, ctx->d_rp_count, ctx->d_rp_words, d_chunks, d_masks, d_rchunks, d_rmasks);
	if (rs_slots > 0) {
		// the rescue: which slots are tried, their combined cells from the store and pass 2's scratch, the groups' Reed-Solomon pass into the
		// slot staging, and the tried runs' rows over k_repeat_end's
		cimbar_hip_ctx::ScratchSet& p2 = ctx->cur();
		HIPCHK(hipMemsetAsync(ctx->d_rs_tap, 0xFF, sizeof(int32_t) * N, st));
		if (salvage) {
			// (d_gcount counts the partials too, for the cells kernel and the taps; the row is made from the full members: d_sv_full)
			hipLaunchKernelGGL(k_rescue_tried_salvage, dim3((rs_slots + 255) / 256), dim3(256), 0, st, ctx->d_rs_count, rs_slots, ctx->d_rs_run, ctx->d_gmem, ctx->d_rp_count,
			                   d_masks, ctx->d_sv_part, ctx->d_gcount, ctx->d_sv_full, ctx->d_gdisp);
			hipLaunchKernelGGL(k_group_cells_salvage, dim3(GC_BLOCKS, rs_slots), dim3(256), 0, st, p2.d_plane, ctx->tb, p2.d_symbols, p2.d_colors, p2.d_drift, p2.d_flood,
			                   ctx->d_gmem, ctx->d_gcount, ctx->d_sv_full, ctx->d_sv_part, ctx->tb_stitch_line, ctx->d_rs_count, ctx->d_rs_map, ctx->d_gsym, ctx->d_gcol,
			                   ctx->d_gmargin, ctx->d_gdisp, rescue_store(ctx));
		} else {
			hipLaunchKernelGGL(k_rescue_tried, dim3((rs_slots + 255) / 256), dim3(256), 0, st, ctx->d_rs_count, rs_slots, ctx->d_rs_run, ctx->d_gmem, ctx->d_rp_count, d_masks,
			                   ctx->d_gcount, ctx->d_gdisp);
			hipLaunchKernelGGL(k_group_cells_rescue, dim3(GC_BLOCKS, rs_slots), dim3(256), 0, st, p2.d_plane, ctx->tb, p2.d_symbols, p2.d_colors, p2.d_drift, p2.d_flood,
			                   ctx->d_gmem, ctx->d_gcount, ctx->d_rs_count, ctx->d_rs_map, ctx->d_gsym, ctx->d_gcol, ctx->d_gmargin, ctx->d_gdisp, rescue_store(ctx));
		}
		launch_live_rs(ctx, st, rs_slots, ctx->d_gsym, ctx->d_gcol, ctx->d_grs_ok, ctx->d_rs_count, ctx->d_gdisp, ctx->d_gchunks);
		hipLaunchKernelGGL(k_group_end_rescue, dim3(rs_slots), dim3(256), 0, st, ctx->d_gsym, ctx->d_gmargin, ctx->tb, ctx->d_gmem, salvage ? ctx->d_sv_full.get() : ctx->d_gcount.get(), ctx->d_rs_count,
		                   ctx->d_grs_ok, d_chunks, d_masks, ctx->d_gdisp, ctx->d_gchunks, ctx->d_gmasks, (!LEGACY && ctx->er_sym > 0) ? 1 : 0, erasure_max(ctx),
		                   ctx->d_rs_run, d_rchunks, d_rmasks, ctx->d_rs_tap);
	}
	HIPCHK(hipGetLastError());
	const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
	if (oa.runs_out) HIPCHK(hipMemcpyAsync(oa.runs_out, ctx->d_rp_runs, sizeof(int) * N, kind, st));
	if (oa.roles) HIPCHK(hipMemcpyAsync(oa.roles, ctx->d_rp_roles, sizeof(int) * N, kind, st));
	auto done = [&]() {
		ctx->rp_n = n;
		ctx->rp_stream = os != nullptr;
		ctx->rs_state = (ctx->rs_on != 0 && !os) ? (rs_slots > 0 ? 2 : 1) : 0;
		ctx->rs_slots = rs_slots;
		ctx->rt_state = tear;
		ctx->sv_state = salvage;
		if (os) { os->cur ^= 1; os->carried = true; }
	};
	if (dev) {
		if (oa.n_runs) HIPCHK(hipMemcpyAsync(oa.n_runs, d_words + (os ? (int)RPC_RUNS : 0), sizeof(int), kind, st));
		if (os && oa.continued) HIPCHK(hipMemcpyAsync(oa.continued, d_words + RPC_CONT, sizeof(int), kind, st));
		done();
		return 0;
	}
	HIPCHK(hipMemcpyAsync(chunks, d_chunks, N * FRAME_BYTES, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(masks, d_masks, sizeof(uint32_t) * N, hipMemcpyDeviceToHost, st));
	if (oa.rchunks) HIPCHK(hipMemcpyAsync(oa.rchunks, d_rchunks, N * FRAME_BYTES, hipMemcpyDeviceToHost, st));
	if (oa.rmasks) HIPCHK(hipMemcpyAsync(oa.rmasks, d_rmasks, sizeof(uint32_t) * N, hipMemcpyDeviceToHost, st));
	if (os) HIPCHK(hipMemcpyAsync(h_words, d_words, sizeof(int) * RP_CALL_WORDS, hipMemcpyDeviceToHost, st));
	if (tear) HIPCHK(hipMemcpyAsync(h_words, d_words, sizeof(int), hipMemcpyDeviceToHost, st));   // the run count: list 1 no longer tells it
	HIPCHK(hipStreamSynchronize(st));
	done();
	const int n_runs = (os || tear) ? ((volatile int*)h_words)[os ? (int)RPC_RUNS : 0] : len1;
	if (oa.n_runs) *oa.n_runs = n_runs;
	if (os && oa.continued) *oa.continued = ((volatile int*)h_words)[RPC_CONT];
	return n_runs;
}

// the once entry points, over frames (cap == nullptr) or captures: oa as the caller gave it (check_once, first of all checks, resolves the two parameters)
int64_t once_call(cimbar_hip_ctx* ctx, CaptureIn* cap, const uint8_t* img, int n, int img_mem, int preprocess, int color_correction, uint8_t* chunks,
                  uint32_t* masks, OnceArgs oa, int out_mem, void* hip_stream)
{
	const std::string name = call_name(cap, oa.stream ? "_once_stream" : "_once");
	const char* who = name.c_str();
	if (int r = check_once(ctx, who, oa)) return r;
	hipStream_t st;
	if (int r = begin_decode(ctx, who, cap, img, n, cap ? "img_mem" : "rgb_mem", img_mem, chunks && masks, out_mem, hip_stream, false, &st)) return r;
	// (a stream call waits for the one before in front of the staging copy: the call before may still be decoding out of d_rgb)
	if (oa.stream) if (int r = begin_once_stream(ctx, st)) return r;
	// (... and every exit from here on, failed or not, goes through end_once_stream)
	const int64_t rc = [&]() -> int64_t {
		FrameSource fs;
		if (int r = cap ? captures_source(ctx, st, *cap, img, n, img_mem, preprocess, out_mem, &fs) : frames_source(ctx, st, img, n, img_mem, preprocess, &fs)) return r;
		return once_impl(ctx, st, fs, n, color_correction, chunks, masks, oa, out_mem);
	}();
	return oa.stream ? end_once_stream(ctx, st, rc) : rc;
}

}  // namespace

int64_t cimbar_hip_decode_batch_once(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                     int min_agree_permille, int max_run, uint8_t* chunks, uint32_t* masks, int* runs_out, int* roles,
                                     uint8_t* rchunks, uint32_t* rmasks, int* n_runs, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return once_call(ctx, nullptr, rgb, n, rgb_mem, should_preprocess, color_correction, chunks, masks,
	                 OnceArgs{min_agree_permille, max_run, runs_out, roles, rchunks, rmasks, n_runs}, out_mem, hip_stream);
}

int64_t cimbar_hip_scan_extract_decode_batch_once_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n,
                                                      int img_mem, int preprocess, int color_correction, int min_agree_permille, int max_run,
                                                      uint8_t* chunks, uint32_t* masks, int* status, int* runs_out, int* roles, uint8_t* rchunks,
                                                      uint32_t* rmasks, int* n_runs, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	CaptureIn cap{width, height, format, status};
	return once_call(ctx, &cap, img, n, img_mem, preprocess, color_correction, chunks, masks,
	                 OnceArgs{min_agree_permille, max_run, runs_out, roles, rchunks, rmasks, n_runs}, out_mem, hip_stream);
}

int64_t cimbar_hip_decode_batch_once_stream(cimbar_hip_ctx* ctx, const uint8_t* rgb, int n, int rgb_mem, int should_preprocess, int color_correction,
                                            int min_agree_permille, int max_run, uint8_t* chunks, uint32_t* masks, int* runs_out, int* roles,
                                            uint8_t* rchunks, uint32_t* rmasks, int* n_runs, int* continued, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	return once_call(ctx, nullptr, rgb, n, rgb_mem, should_preprocess, color_correction, chunks, masks,
	                 OnceArgs{min_agree_permille, max_run, runs_out, roles, rchunks, rmasks, n_runs, true, continued}, out_mem, hip_stream);
}

int64_t cimbar_hip_scan_extract_decode_batch_once_stream_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n,
                                                             int img_mem, int preprocess, int color_correction, int min_agree_permille, int max_run,
                                                             uint8_t* chunks, uint32_t* masks, int* status, int* runs_out, int* roles,
                                                             uint8_t* rchunks, uint32_t* rmasks, int* n_runs, int* continued, int out_mem,
                                                             void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	CaptureIn cap{width, height, format, status};
	return once_call(ctx, &cap, img, n, img_mem, preprocess, color_correction, chunks, masks,
	                 OnceArgs{min_agree_permille, max_run, runs_out, roles, rchunks, rmasks, n_runs, true, continued}, out_mem, hip_stream);
}

// wait for the once-stream calls issued so far and forget the carry: the next one's capture 0 starts a run
int cimbar_hip_once_stream_reset(cimbar_hip_ctx* ctx)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (!ctx->ostream) return 0;
	OnceStream& s = *ctx->ostream;
	HIPCHK(hipSetDevice(ctx->device));
	if (s.used) HIPCHK(hipEventSynchronize(s.ev_last));
	if (s.words) HIPCHK(hipMemset(s.words, 0, sizeof(uint32_t) * 2 * RP_CARRY_WORDS));
	s.carried = false;
	return 0;
}

int cimbar_hip_set_template(cimbar_hip_ctx* ctx, const uint8_t* rgb_template, int mem)
{
	if (!ctx || !rgb_template) return CIMBAR_HIP_EINVAL;
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(ctx->d_template.ensure(FRAME_RGB));
	HIPCHK(hipMemcpy(ctx->d_template, rgb_template, FRAME_RGB, mem == CIMBAR_HIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
	return 0;
}

int cimbar_hip_encode_batch(cimbar_hip_ctx* ctx, const uint8_t* payload, int n, int payload_mem, uint8_t* rgb_out, int rgb_mem,
                            void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (!payload || !rgb_out || n <= 0) { ctx->err = "encode_batch: null buffer or n <= 0"; return CIMBAR_HIP_EINVAL; }
	if (!ctx->d_template) { ctx->err = "encode_batch: call cimbar_hip_set_template first"; return CIMBAR_HIP_EINVAL; }
	hipStream_t st;
	if (int r = begin_call(ctx, "encode_batch", "payload_mem", payload_mem, "rgb_mem", rgb_mem, hip_stream, &st)) return r;
	if (int r = ensure_capacity(ctx, n)) return r;
	const uint8_t* d_payload = nullptr;
	if (int r = stage_input(ctx, st, ctx->d_payload, payload, (size_t)n * FRAME_BYTES, payload_mem, &d_payload)) return r;
	uint8_t* d_out = nullptr;
	if (int r = stage_output(ctx, ctx->d_rgb, rgb_out, (size_t)n * FRAME_RGB, rgb_mem, &d_out)) return r;
	cimbar_hip_ctx::ScratchSet& cur = ctx->cur();
	uint8_t* d_stream = nullptr;
	if (LEGACY) {   // the RS-encoded stream as bytes, cut into 6-bit cells by a second kernel (the plane scratch is free here and large enough)
		static_assert((size_t)ALL_BLOCKS * RS_BLOCK <= (size_t)PLANE_WORDS * 4, "the encoded stream fits the bit-plane scratch");
		d_stream = reinterpret_cast<uint8_t*>(cur.d_plane.get());
	}
	hipLaunchKernelGGL(k_rs_encode, dim3((n * ALL_BLOCKS + 3) / 4), dim3(256), 0, st, d_payload, ctx->tb, ctx->d_gen_log, n, cur.d_symbols, cur.d_colors, d_stream);
	if (LEGACY) hipLaunchKernelGGL(k_fields_legacy, dim3((NCELLS + 255) / 256, n), dim3(256), 0, st, d_stream, ctx->tb, n, cur.d_symbols, cur.d_colors);
	hipLaunchKernelGGL(k_render, dim3((IMG_H + 3) / 4, n), dim3(256), 0, st, cur.d_symbols, cur.d_colors, ctx->d_template, d_out);
	HIPCHK(hipGetLastError());
	if (rgb_mem == CIMBAR_HIP_MEM_HOST) {
		HIPCHK(hipMemcpyAsync(rgb_out, d_out, (size_t)n * FRAME_RGB, hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
	}
	return 0;
}

int cimbar_hip_set_erasure_decode(cimbar_hip_ctx* ctx, int sym_distance, int colour_margin, int max_erasures)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (LEGACY && sym_distance > 0) { ctx->err = "set_erasure_decode: modes 4 and 8 carry one coupled stream; erasure decoding covers the symbol blocks of modes 68 / 67 / 66"; return CIMBAR_HIP_EINVAL; }
	if (sym_distance > 64 || max_erasures > RS_PARITY) { ctx->err = "set_erasure_decode: sym_distance <= 64, max_erasures <= the parity bytes"; return CIMBAR_HIP_EINVAL; }
	// (read when a batch is enqueued: batches already issued keep the setting they were issued with)
	ctx->er_sym = sym_distance > 0 ? sym_distance : 0;
	ctx->er_col = colour_margin < 0 ? -1 : colour_margin;
	ctx->er_max = max_erasures < 0 ? -1 : max_erasures;
	return 0;
}

int cimbar_hip_get_erasure_decode(cimbar_hip_ctx* ctx, int* sym_distance, int* colour_margin, int* max_erasures)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (sym_distance) *sym_distance = ctx->er_sym;
	if (colour_margin) *colour_margin = ctx->er_col;
	if (max_erasures) *max_erasures = erasure_max(ctx);
	return ctx->er_sym > 0 ? 1 : 0;
}

int cimbar_hip_set_colour_erasure_decode(cimbar_hip_ctx* ctx, int colour_margin, int max_erasures)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (LEGACY && colour_margin > 0) { ctx->err = "set_colour_erasure_decode: modes 4 and 8 carry one coupled stream; colour erasure decoding covers the colour blocks of modes 68 / 67 / 66"; return CIMBAR_HIP_EINVAL; }
	if (max_erasures > RS_PARITY) { ctx->err = "set_colour_erasure_decode: max_erasures <= the parity bytes"; return CIMBAR_HIP_EINVAL; }
	// (read when a batch is enqueued: batches already issued keep the setting they were issued with)
	ctx->ec_margin = colour_margin > 0 ? colour_margin : 0;
	ctx->ec_max = max_erasures < 0 ? -1 : max_erasures;
	if (ctx->ec_margin > 0 && ctx->cur().cap > 0) {
		// the margin buffer (CIMBAR_HIP_TAP_COLOUR_MARGIN) exists from the first time the setting is on; a context that has not decoded yet gets it with its scratch
		HIPCHK(hipSetDevice(ctx->device));
		if (int r = ensure_margin_capacity(ctx, ctx->cur())) return r;
	}
	return 0;
}

int cimbar_hip_get_colour_erasure_decode(cimbar_hip_ctx* ctx, int* colour_margin, int* max_erasures)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (colour_margin) *colour_margin = ctx->ec_margin;
	if (max_erasures) *max_erasures = colour_erasure_max(ctx);
	return ctx->ec_margin > 0 ? 1 : 0;
}

int cimbar_hip_set_relaxed_flood(cimbar_hip_ctx* ctx, int threshold, int fallback)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (threshold < -1 || threshold > FR_THRESHOLD_MAX) { ctx->err = "set_relaxed_flood: threshold -1 (off) or 0 .. 32"; return CIMBAR_HIP_EINVAL; }
	if (LEGACY && threshold >= 0) { ctx->err = "set_relaxed_flood: modes 4 and 8 decode their one RS stream after the colour pass; there is nothing to check a relaxed flood against"; return CIMBAR_HIP_EINVAL; }
	HIPCHK(hipSetDevice(ctx->device));
	if (threshold >= 0 && !ctx->d_rf_stats) HIPCHK(ctx->d_rf_stats.reserve(4));
	if (ctx->d_rf_stats) {
		// (the counts of batches still in flight belong to the old setting)
		HIPCHK(hipDeviceSynchronize());
		HIPCHK(hipMemset(ctx->d_rf_stats, 0, 4 * sizeof(unsigned long long)));
	}
	// (read when a batch is enqueued: batches already issued keep the setting they were issued with)
	ctx->rf_threshold = threshold;
	ctx->rf_fallback = threshold >= 0 && fallback ? 1 : 0;
	return 0;
}

int cimbar_hip_get_relaxed_flood(cimbar_hip_ctx* ctx, int* threshold, int* fallback)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (threshold) *threshold = ctx->rf_threshold;
	if (fallback) *fallback = ctx->rf_fallback;
	return ctx->rf_threshold >= 0 ? 1 : 0;
}

int cimbar_hip_relaxed_flood_stats(cimbar_hip_ctx* ctx, int64_t out[4])
{
	if (!ctx || !out) return CIMBAR_HIP_EINVAL;
	for (int k = 0; k < 4; ++k) out[k] = 0;
	if (!ctx->d_rf_stats) return 0;
	unsigned long long t[4];
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(t, ctx->d_rf_stats, sizeof t, hipMemcpyDeviceToHost));
	for (int k = 0; k < 4; ++k) out[k] = (int64_t)t[k];
	return 0;
}

int cimbar_hip_set_group_colour_vote(cimbar_hip_ctx* ctx, int on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (LEGACY && on) { ctx->err = "set_group_colour_vote: modes 4 and 8 carry one coupled stream; the colour vote covers the colour chunks of modes 68 / 67 / 66"; return CIMBAR_HIP_EINVAL; }
	// (read when a combined batch is enqueued: batches already issued keep the setting they were issued with)
	ctx->gcv_on = on ? 1 : 0;
	return 0;
}

int cimbar_hip_get_group_colour_vote(cimbar_hip_ctx* ctx, int* on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (on) *on = ctx->gcv_on;
	return 0;
}

int cimbar_hip_set_once_rescue(cimbar_hip_ctx* ctx, int on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (LEGACY && on) { ctx->err = "set_once_rescue: modes 4 and 8 have no once-calls to govern; repeat-capture skipping covers modes 68 / 67 / 66"; return CIMBAR_HIP_EINVAL; }
	// (read when a plain once-call is enqueued: calls already issued keep the setting they were issued with)
	ctx->rs_on = on ? 1 : 0;
	return 0;
}

int cimbar_hip_get_once_rescue(cimbar_hip_ctx* ctx, int* on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (on) *on = ctx->rs_on;
	return 0;
}

int cimbar_hip_set_once_tear_skip(cimbar_hip_ctx* ctx, int axis, int line_permille, int min_side)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (axis < -1 || axis > 2) { ctx->err = "set_once_tear_skip: axis must be -1 (off), 0, 1 or 2"; return CIMBAR_HIP_EINVAL; }
	if (axis == -1) { ctx->rt_axis = -1; ctx->rt_line = RT_LINE_DEFAULT; ctx->rt_side = RT_SIDE_DEFAULT; return 0; }
	if (LEGACY) { ctx->err = "set_once_tear_skip: modes 4 and 8 have no once-calls to govern; repeat-capture skipping covers modes 68 / 67 / 66"; return CIMBAR_HIP_EINVAL; }
	if (line_permille > 1000) { ctx->err = "set_once_tear_skip: line_permille above 1000"; return CIMBAR_HIP_EINVAL; }
	if (line_permille <= 0) line_permille = RT_LINE_DEFAULT;
	if (min_side <= 0) min_side = RT_SIDE_DEFAULT;
	const int L = axis == 2 ? (stitch_lines(0) < stitch_lines(1) ? stitch_lines(0) : stitch_lines(1)) : stitch_lines(axis);
	if (min_side > L / 2) { ctx->err = "set_once_tear_skip: 2 * min_side above the lines of the axis"; return CIMBAR_HIP_EINVAL; }
	// (read when a plain once-call is enqueued: calls already issued keep the setting they were issued with)
	ctx->rt_axis = axis; ctx->rt_line = line_permille; ctx->rt_side = min_side;
	return 0;
}

int cimbar_hip_get_once_tear_skip(cimbar_hip_ctx* ctx, int* axis, int* line_permille, int* min_side)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (axis) *axis = ctx->rt_axis;
	if (line_permille) *line_permille = ctx->rt_line;
	if (min_side) *min_side = ctx->rt_side;
	return 0;
}

int cimbar_hip_set_once_tear_salvage(cimbar_hip_ctx* ctx, int on, int guard_lines)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (guard_lines < -1 || guard_lines > RV_GUARD_MAX) { ctx->err = "set_once_tear_salvage: guard_lines must be -1 (the default, 1) or 0 .. 16"; return CIMBAR_HIP_EINVAL; }
	if (LEGACY && on) { ctx->err = "set_once_tear_salvage: modes 4 and 8 have no once-calls to govern; repeat-capture skipping covers modes 68 / 67 / 66"; return CIMBAR_HIP_EINVAL; }
	// (read when a plain once-call is enqueued: calls already issued keep the setting they were issued with)
	ctx->sv_on = on ? 1 : 0;
	ctx->sv_guard = guard_lines < 0 ? RV_GUARD_DEFAULT : guard_lines;
	return 0;
}

int cimbar_hip_get_once_tear_salvage(cimbar_hip_ctx* ctx, int* on, int* guard_lines)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (on) *on = ctx->sv_on;
	if (guard_lines) *guard_lines = ctx->sv_guard;
	return 0;
}

int cimbar_hip_set_stitch_strips(cimbar_hip_ctx* ctx, int strips)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (strips < 1 || strips > STITCH_SMAX) { ctx->err = "set_stitch_strips: strips must be 1 .. 8"; return CIMBAR_HIP_EINVAL; }
	// (read when a stitched call is enqueued: calls already issued keep the setting they were issued with)
	ctx->stitch_strips = strips;
	return 0;
}

int cimbar_hip_get_stitch_strips(cimbar_hip_ctx* ctx, int* strips)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (strips) *strips = ctx->stitch_strips;
	return 0;
}

int cimbar_hip_set_stitch_erasure(cimbar_hip_ctx* ctx, int on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (LEGACY && on) { ctx->err = "set_stitch_erasure: modes 4 and 8 carry one coupled stream; the erasure retries cover modes 68 / 67 / 66"; return CIMBAR_HIP_EINVAL; }
	// (read when a stitched call is enqueued: calls already issued keep the setting they were issued with)
	ctx->stitch_er = on ? 1 : 0;
	return 0;
}

int cimbar_hip_get_stitch_erasure(cimbar_hip_ctx* ctx, int* on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (on) *on = ctx->stitch_er;
	return 0;
}

int cimbar_hip_set_stream_colour_vote(cimbar_hip_ctx* ctx, int on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (LEGACY && on) { ctx->err = "set_stream_colour_vote: modes 4 and 8 carry one coupled stream; the colour vote covers the colour chunks of modes 68 / 67 / 66"; return CIMBAR_HIP_EINVAL; }
	// (a stream samples it in its first call after create / reset and refuses a call that finds it changed: check_combine)
	ctx->sgv_on = on ? 1 : 0;
	return 0;
}

int cimbar_hip_get_stream_colour_vote(cimbar_hip_ctx* ctx, int* on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (on) *on = ctx->sgv_on;
	return 0;
}

int cimbar_hip_rs_decode_erasures(cimbar_hip_ctx* ctx, const uint8_t* blocks, int n, const uint8_t* erasures, const uint8_t* counts, int mem,
                                  uint8_t* msgs, int8_t* status, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (!blocks || !erasures || !counts || !msgs || !status || n <= 0) { ctx->err = "rs_decode_erasures: null buffer or n <= 0"; return CIMBAR_HIP_EINVAL; }
	// (not begin_call: the call touches no scratch set, so it does not wait for the pipelined batches in flight, and its streams are its own -- below)
	if (int r = check_mem_flags(ctx, "rs_decode_erasures", nullptr, 0, "mem", mem)) return r;
	HIPCHK(hipSetDevice(ctx->device));
	const unsigned grid = (unsigned)((n + 3) / 4);
	if (mem == CIMBAR_HIP_MEM_DEVICE) {   // stream-ordered on the caller's stream (the null stream by default); nothing waits
		hipLaunchKernelGGL(k_rs_erasures, dim3(grid), dim3(256), 0, (hipStream_t)hip_stream, blocks, n, erasures, counts, msgs, status);
		HIPCHK(hipGetLastError());
		return 0;
	}
	// host memory: staged through a context-owned device buffer (grown on demand, kept), synchronous. A NULL stream is the context's own
	// stream here, the null stream for device memory: the convention of cimbar_hip_encode_batch / cimbar_hip_decode_batch.
	hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
	const size_t nb = (size_t)n * RS_BLOCK, nm = (size_t)n * RS_DATA, need = 2 * nb + 2 * (size_t)n + nm;
	if (need > ctx->d_er_buf.capacity()) HIPCHK(hipStreamSynchronize(st));   // (a previous call's copies on another stream are complete: every host-memory call synchronises)
	HIPCHK(ctx->d_er_buf.reserve(need));
	uint8_t* d = ctx->d_er_buf;
	uint8_t *d_blocks = d, *d_er = d + nb, *d_counts = d + 2 * nb, *d_msgs = d_counts + n;
	int8_t* d_status = reinterpret_cast<int8_t*>(d_msgs + nm);
	hipError_t e = hipMemcpyAsync(d_blocks, blocks, nb, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(d_er, erasures, nb, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(d_counts, counts, (size_t)n, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) {
		hipLaunchKernelGGL(k_rs_erasures, dim3(grid), dim3(256), 0, st, d_blocks, n, d_er, d_counts, d_msgs, d_status);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(msgs, d_msgs, nm, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(status, d_status, (size_t)n, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	HIPCHK(e);
	return 0;
}

int64_t cimbar_hip_tap(cimbar_hip_ctx* ctx, int what, void* out, size_t out_bytes)
{
	if (!ctx || !out) return CIMBAR_HIP_EINVAL;
	if (what == CIMBAR_HIP_TAP_FLOOD_LAUNCH) {
		// which exact-replay launches the last enqueue() made: host bookkeeping, no device work and no wait (batches may still be in flight)
		if (ctx->last_n <= 0) { ctx->err = "tap: no batch has been decoded on this context yet"; return CIMBAR_HIP_EINVAL; }
		const size_t bytes = sizeof(int32_t) * 7 * (size_t)(1 + ctx->flood_launch_n);
		if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
		const int32_t head[7] = {ctx->flood_launch_top, ctx->flood_cap, ctx->flood_launch_n, 0, 0, 0, 0};
		std::memcpy(out, head, sizeof head);
		std::memcpy((int32_t*)out + 7, ctx->flood_launch, bytes - sizeof head);
		return (int64_t)bytes;
	}
	if (what == CIMBAR_HIP_TAP_SCAN_PATH) {
		// which kernels answered the last anchor search, per capture: the fast kernels' overflow flag and the status the slow path left
		if (ctx->scan_n <= 0) { ctx->err = "tap: no capture has been searched for anchors on this context yet"; return CIMBAR_HIP_EINVAL; }
		const size_t m = (size_t)ctx->scan_n;
		if (out_bytes < m * sizeof(int32_t)) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
		HIPCHK(hipSetDevice(ctx->device));
		HIPCHK(hipDeviceSynchronize());
		std::vector<int> ovf(m), status(m);
		HIPCHK(hipMemcpy(ovf.data(), ctx->d_scan_ovf, sizeof(int) * m, hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy2D(status.data(), sizeof(int), &ctx->d_scan_res[0].status, sizeof(ScanResult), sizeof(int), m, hipMemcpyDeviceToHost));
		for (size_t k = 0; k < m; ++k) ((int32_t*)out)[k] = status[k] < 0 ? 2 : (ovf[k] ? 1 : 0);
		return (int64_t)(m * sizeof(int32_t));
	}
	if (what == CIMBAR_HIP_TAP_SCAN_GRAY || what == CIMBAR_HIP_TAP_SCAN_HIST || what == CIMBAR_HIP_TAP_SCAN_THRESHOLD) {
		// what the stage in front of that search left: blurred gray planes, their histograms, the Otsu thresholds
		if (ctx->scan_n <= 0) { ctx->err = "tap: no capture has been searched for anchors on this context yet"; return CIMBAR_HIP_EINVAL; }
		const size_t m = (size_t)ctx->scan_n;
		const void* src = what == CIMBAR_HIP_TAP_SCAN_GRAY ? (const void*)ctx->d_ex_gray : (what == CIMBAR_HIP_TAP_SCAN_HIST ? (const void*)ctx->d_ex_hist : (const void*)ctx->d_ex_thr);
		const size_t bytes = what == CIMBAR_HIP_TAP_SCAN_GRAY ? m * ctx->scan_w * ctx->scan_h : (what == CIMBAR_HIP_TAP_SCAN_HIST ? m * 256 * sizeof(uint32_t) : m * sizeof(int32_t));
		if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
		HIPCHK(hipSetDevice(ctx->device));
		HIPCHK(hipDeviceSynchronize());
		HIPCHK(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
		return (int64_t)bytes;
	}
	if (what == CIMBAR_HIP_TAP_STITCH_CARRY) {
		// what the next stitched-stream call's row 0 is held against: the carried symbols, then the carried colours
		if (!ctx->sstream || !ctx->sstream->carried) { ctx->err = "tap: nothing is carried (no stitched-stream call since create / cimbar_hip_stitch_stream_reset)"; return CIMBAR_HIP_EINVAL; }
		if (out_bytes < (size_t)2 * NCELLS) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
		const StitchStream& s = *ctx->sstream;
		HIPCHK(hipSetDevice(ctx->device));
		HIPCHK(hipDeviceSynchronize());
		HIPCHK(hipMemcpy(out, s.symbols + (size_t)s.cur * SS_CELLS, NCELLS, hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy((uint8_t*)out + NCELLS, s.colors + (size_t)s.cur * SS_CELLS, NCELLS, hipMemcpyDeviceToHost));
		return (int64_t)2 * NCELLS;
	}
	if (what == CIMBAR_HIP_TAP_REPEAT_CARRY) {
		// what the next once-stream call's capture 0 is held against: the carried signature, then {usable, len, P}
		if (!ctx->ostream || !ctx->ostream->carried) { ctx->err = "tap: nothing is carried (no once-stream call since create / cimbar_hip_once_stream_reset)"; return CIMBAR_HIP_EINVAL; }
		const size_t bytes = (size_t)NCELLS + 3 * sizeof(uint32_t);
		if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
		const OnceStream& s = *ctx->ostream;
		HIPCHK(hipSetDevice(ctx->device));
		HIPCHK(hipDeviceSynchronize());
		HIPCHK(hipMemcpy(out, s.sig + (size_t)s.cur * RP_CARRY_SIG, NCELLS, hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy((uint8_t*)out + NCELLS, s.words + (size_t)s.cur * RP_CARRY_WORDS, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
		return (int64_t)bytes;
	}
	if (what == CIMBAR_HIP_TAP_REPEAT_SIG || what == CIMBAR_HIP_TAP_REPEAT_AGREE) {
		// what the last once-call grouped its captures by (its n, not the length of the list its last pass decoded)
		if (ctx->rp_n <= 0) { ctx->err = "tap: no once-call has run on this context yet (cimbar_hip_decode_batch_once / _scan_extract_decode_batch_once_fmt)"; return CIMBAR_HIP_EINVAL; }
		const size_t m = (size_t)ctx->rp_n;
		const size_t bytes = what == CIMBAR_HIP_TAP_REPEAT_SIG ? m * NCELLS : (ctx->rp_stream ? m : m - 1) * sizeof(uint32_t);   // (a once-stream call: entry 0 against the carry)
		if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
		HIPCHK(hipSetDevice(ctx->device));
		HIPCHK(hipDeviceSynchronize());
		if (bytes) HIPCHK(hipMemcpy(out, what == CIMBAR_HIP_TAP_REPEAT_SIG ? (const void*)ctx->d_rp_sig.get() : (const void*)ctx->d_rp_agree.get(), bytes, hipMemcpyDeviceToHost));
		return (int64_t)bytes;
	}
	if (what == CIMBAR_HIP_TAP_ONCE_TEAR) {
		// tear skipping in the last plain once-call: one record per capture
		if (ctx->rp_n <= 0 || !ctx->rt_state) { ctx->err = "tap: the last once-call was not a plain one with tear skipping on (cimbar_hip_set_once_tear_skip)"; return CIMBAR_HIP_EINVAL; }
		const size_t bytes = (size_t)ctx->rp_n * 4 * sizeof(int32_t);
		if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
		HIPCHK(hipSetDevice(ctx->device));
		HIPCHK(hipDeviceSynchronize());
		HIPCHK(hipMemcpy(out, ctx->d_rt_tap, bytes, hipMemcpyDeviceToHost));
		return (int64_t)bytes;
	}
	if (what == CIMBAR_HIP_TAP_ONCE_SALVAGE) {
		// tear salvage in the last plain once-call: per run slot the partials of a tried run, composed from the slots' rows
		if (ctx->rp_n <= 0 || !ctx->sv_state) { ctx->err = "tap: the last once-call was not a plain one in which tear salvage was effective (cimbar_hip_set_once_tear_salvage)"; return CIMBAR_HIP_EINVAL; }
		const size_t m = (size_t)ctx->rp_n, S = ctx->rs_state == 2 ? (size_t)ctx->rs_slots : 0;
		if (out_bytes < m * 8 * sizeof(int32_t)) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
		HIPCHK(hipSetDevice(ctx->device));
		HIPCHK(hipDeviceSynchronize());
		int32_t* o = (int32_t*)out;
		for (size_t r = 0; r < m; ++r) for (int h = 0; h < 2; ++h) { o[r * 8 + 4 * h] = o[r * 8 + 4 * h + 1] = -1; o[r * 8 + 4 * h + 2] = o[r * 8 + 4 * h + 3] = 0; }
		if (S) {
			int live = 0;
			std::vector<int> cnt(S), run(S);
			std::vector<int32_t> part(S * 8);
			HIPCHK(hipMemcpy(&live, ctx->d_rs_count, sizeof(int), hipMemcpyDeviceToHost));
			HIPCHK(hipMemcpy(cnt.data(), ctx->d_gcount, sizeof(int) * S, hipMemcpyDeviceToHost));
			HIPCHK(hipMemcpy(run.data(), ctx->d_rs_run, sizeof(int) * S, hipMemcpyDeviceToHost));
			HIPCHK(hipMemcpy(part.data(), ctx->d_sv_part, sizeof(int32_t) * 8 * S, hipMemcpyDeviceToHost));
			for (size_t s = 0; s < S && s < (size_t)live; ++s)
				if (cnt[s] > 0 && run[s] >= 0 && (size_t)run[s] < m) std::memcpy(o + (size_t)run[s] * 8, &part[s * 8], 8 * sizeof(int32_t));
		}
		return (int64_t)(m * 8 * sizeof(int32_t));
	}
	if (what == CIMBAR_HIP_TAP_ONCE_RESCUE || what == CIMBAR_HIP_TAP_ONCE_RESCUE_CELLS) {
		// the run rescue of the last plain once-call: per run slot what it added, and the combined cells of the tried runs, in run order
		if (ctx->rp_n <= 0 || ctx->rs_state == 0) { ctx->err = "tap: the last once-call was not a plain one with the run rescue on (cimbar_hip_set_once_rescue)"; return CIMBAR_HIP_EINVAL; }
		const size_t m = (size_t)ctx->rp_n, S = ctx->rs_state == 2 ? (size_t)ctx->rs_slots : 0;
		HIPCHK(hipSetDevice(ctx->device));
		HIPCHK(hipDeviceSynchronize());
		if (what == CIMBAR_HIP_TAP_ONCE_RESCUE) {
			if (out_bytes < m * sizeof(int32_t)) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
			if (S) HIPCHK(hipMemcpy(out, ctx->d_rs_tap, m * sizeof(int32_t), hipMemcpyDeviceToHost));
			else std::memset(out, 0xFF, m * sizeof(int32_t));
			return (int64_t)(m * sizeof(int32_t));
		}
		std::vector<int> cnt(S);
		int live = 0;
		if (S) {
			HIPCHK(hipMemcpy(&live, ctx->d_rs_count, sizeof(int), hipMemcpyDeviceToHost));
			HIPCHK(hipMemcpy(cnt.data(), ctx->d_gcount, sizeof(int) * S, hipMemcpyDeviceToHost));
		}
		size_t tried = 0;
		for (size_t s = 0; s < S && s < (size_t)live; ++s) tried += cnt[s] > 0 ? 1 : 0;
		if (out_bytes < tried * NCELLS) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
		std::vector<uint8_t> sym(NCELLS), col(NCELLS);
		uint8_t* o = (uint8_t*)out;
		for (size_t s = 0; s < S && s < (size_t)live; ++s) {
			if (cnt[s] <= 0) continue;
			HIPCHK(hipMemcpy(sym.data(), ctx->d_gsym + s * NCELLS, NCELLS, hipMemcpyDeviceToHost));
			HIPCHK(hipMemcpy(col.data(), ctx->d_gcol + s * NCELLS, NCELLS, hipMemcpyDeviceToHost));
			for (size_t k = 0; k < (size_t)NCELLS; ++k) o[k] = (uint8_t)((col[k] << 4) | (sym[k] & 15u));
			o += NCELLS;
		}
		return (int64_t)(tried * NCELLS);
	}
	if (ctx->last_n <= 0) { ctx->err = "tap: no batch has been decoded on this context yet"; return CIMBAR_HIP_EINVAL; }
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipDeviceSynchronize());
	const size_t n = (size_t)ctx->last_n;
	cimbar_hip_ctx::ScratchSet& cur = ctx->cur();
	const void* src = nullptr;
	size_t bytes = 0;
	switch (what) {
		case CIMBAR_HIP_TAP_BITPLANE: {
			bytes = n * (size_t)IMG_W * IMG_H / 8;                     // CimbReader::_grayscale's layout: the bits of a frame back to back
			if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
			DevBuf<uint8_t> tmp;
			HIPCHK(tmp.reserve(bytes));
			size_t nw = bytes / 4;
			hipLaunchKernelGGL(k_plane_bytes, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, ctx->stream, cur.d_plane, tmp, nw);
			hipError_t e = hipMemcpyAsync(out, tmp, bytes, hipMemcpyDeviceToHost, ctx->stream);
			if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
			HIPCHK(e);
			return (int64_t)bytes;
		}
		case CIMBAR_HIP_TAP_SYMBOLS: src = cur.d_symbols; bytes = n * NCELLS; break;
		case CIMBAR_HIP_TAP_COLORS: src = cur.d_colors; bytes = n * NCELLS; break;
		case CIMBAR_HIP_TAP_DRIFT: src = cur.d_drift; bytes = n * NCELLS * 2; break;
		case CIMBAR_HIP_TAP_RS_OK: src = cur.d_rs_ok; bytes = n * ALL_BLOCKS; break;
		case CIMBAR_HIP_TAP_CCM: src = cur.d_ccm_used; bytes = n * 10 * sizeof(float); break;
		case CIMBAR_HIP_TAP_CELL_MEANS: src = cur.d_cellmean; bytes = n * GRID_CELLS * sizeof(uint32_t); break;
		case CIMBAR_HIP_TAP_FLOOD: {
			bytes = n;
			if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
			std::vector<uint32_t> tmp(n);
			HIPCHK(hipMemcpy(tmp.data(), cur.d_flood, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
			for (size_t k = 0; k < n; ++k) ((uint8_t*)out)[k] = tmp[k] ? 1 : 0;
			return (int64_t)bytes;
		}
		case CIMBAR_HIP_TAP_FLOOD_INFO: {
			bytes = n * sizeof(uint32_t);
			if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
			std::vector<uint32_t> fl(n);
			HIPCHK(hipMemcpy(fl.data(), cur.d_flood, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
			HIPCHK(hipMemcpy(out, cur.d_flood + cur.cap, bytes, hipMemcpyDeviceToHost));
			for (size_t k = 0; k < n; ++k) if (!fl[k]) ((uint32_t*)out)[k] = 0xFFFFFFFFu;   // frame never flagged: the batch-parallel flood did not look at it
			return (int64_t)bytes;
		}
		case CIMBAR_HIP_TAP_FLOOD_ROUNDS: {
			bytes = n * sizeof(uint32_t);
			if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
			if (!ctx->rf_valid) { std::memset(out, 0, bytes); return (int64_t)bytes; }   // the batch ran without the relaxed flood: no frame took rounds
			HIPCHK(hipMemcpy(out, cur.d_flood + 2 * cur.cap, bytes, hipMemcpyDeviceToHost));
			return (int64_t)bytes;
		}
		case CIMBAR_HIP_TAP_FLOOD_PATH: {
			bytes = n;
			if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
			std::vector<uint32_t> tmp(n);
			HIPCHK(hipMemcpy(tmp.data(), cur.d_flood, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
			for (size_t k = 0; k < n; ++k) ((uint8_t*)out)[k] = (uint8_t)tmp[k];
			return (int64_t)bytes;
		}
		case CIMBAR_HIP_TAP_FLOOD_VERIFY: {
			bytes = n * sizeof(uint32_t);
			if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
			if (!ctx->flood_verify || !ctx->d_vflag || (size_t)ctx->vcap < n) { std::memset(out, 0xFF, bytes); return (int64_t)bytes; }
			HIPCHK(hipDeviceSynchronize());
			HIPCHK(hipMemcpy(out, ctx->d_vflag + ctx->vcap, bytes, hipMemcpyDeviceToHost));
			return (int64_t)bytes;
		}
		case CIMBAR_HIP_TAP_COLOUR_MARGIN: {
			if (!ctx->cm_valid || !cur.d_cmargin || (size_t)cur.cm_cap < n) { ctx->err = "tap: the last batch ran without colour erasure decoding (cimbar_hip_set_colour_erasure_decode)"; return CIMBAR_HIP_EINVAL; }
			bytes = n * NCELLS * sizeof(uint32_t);
			if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
			std::vector<uint32_t> worked(n);
			HIPCHK(hipMemcpy(out, cur.d_cmargin, bytes, hipMemcpyDeviceToHost));
			HIPCHK(hipMemcpy(worked.data(), cur.d_cmargin + (size_t)cur.cm_cap * NCELLS, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
			// frames whose colour chunks were all in the mask: the retry returned at once and computed no margin
			for (size_t k = 0; k < n; ++k) if (!worked[k]) std::memset((uint32_t*)out + k * NCELLS, 0xFF, (size_t)NCELLS * sizeof(uint32_t));
			return (int64_t)bytes;
		}
		case CIMBAR_HIP_TAP_GROUP_CELLS:
		case CIMBAR_HIP_TAP_GROUP_MARGIN:
		case CIMBAR_HIP_TAP_GROUPS: {
			if (!ctx->grp_valid) { ctx->err = "tap: the last batch was not a combined one (cimbar_hip_decode_batch_combined / _scan_extract_decode_batch_combined_fmt)"; return CIMBAR_HIP_EINVAL; }
			int ng = 0;
			HIPCHK(hipMemcpy(&ng, ctx->d_ngroups, sizeof(int), hipMemcpyDeviceToHost));
			const size_t G = (size_t)ng;
			bytes = what == CIMBAR_HIP_TAP_GROUPS ? n * sizeof(int32_t) : G * NCELLS * (what == CIMBAR_HIP_TAP_GROUP_MARGIN ? 2 : 1);
			if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
			if (what == CIMBAR_HIP_TAP_GROUPS) HIPCHK(hipMemcpy(out, ctx->d_groups, bytes, hipMemcpyDeviceToHost));
			else if (what == CIMBAR_HIP_TAP_GROUP_MARGIN) { if (bytes) HIPCHK(hipMemcpy(out, ctx->d_gmargin, bytes, hipMemcpyDeviceToHost)); }
			else if (bytes) {
				std::vector<uint8_t> col(bytes);
				HIPCHK(hipMemcpy(out, ctx->d_gsym, bytes, hipMemcpyDeviceToHost));
				HIPCHK(hipMemcpy(col.data(), ctx->d_gcol, bytes, hipMemcpyDeviceToHost));
				for (size_t k = 0; k < bytes; ++k) ((uint8_t*)out)[k] = (uint8_t)((col[k] << 4) | (((uint8_t*)out)[k] & 15u));
			}
			return (int64_t)bytes;
		}
		case CIMBAR_HIP_TAP_GROUP_COLOUR_MARGIN:
		case CIMBAR_HIP_TAP_GROUP_COLOUR_WEIGHTS: {
			if (!ctx->grp_valid || !ctx->gcv_valid || !ctx->d_gcm || !ctx->d_gcw) { ctx->err = "tap: the last batch was not a combined one with its colour vote on (cimbar_hip_set_group_colour_vote / cimbar_hip_set_stream_colour_vote)"; return CIMBAR_HIP_EINVAL; }
			int ng = 0;
			HIPCHK(hipMemcpy(&ng, ctx->d_ngroups, sizeof(int), hipMemcpyDeviceToHost));
			// (a stream call: the groups that closed in it and its own captures -- a flush without captures has none)
			const size_t n = ctx->gcv_stream_n >= 0 ? (size_t)ctx->gcv_stream_n : (size_t)ctx->last_n;
			const size_t G = (size_t)ng, rows = what == CIMBAR_HIP_TAP_GROUP_COLOUR_MARGIN ? G : n;
			bytes = rows * NCELLS * sizeof(uint32_t);
			if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
			std::vector<uint32_t> disp(G);
			std::vector<int> grp(n);
			if (G) HIPCHK(hipMemcpy(disp.data(), ctx->d_gdisp, sizeof(uint32_t) * G, hipMemcpyDeviceToHost));
			if (n) HIPCHK(hipMemcpy(grp.data(), ctx->d_groups, sizeof(int) * n, hipMemcpyDeviceToHost));
			if (bytes) HIPCHK(hipMemcpy(out, what == CIMBAR_HIP_TAP_GROUP_COLOUR_MARGIN ? ctx->d_gcm.get() : ctx->d_gcw.get(), bytes, hipMemcpyDeviceToHost));
			// a group whose members agree on every cell was skipped by the vote: no margin; its members, and captures in no group, gave no weight
			if (what == CIMBAR_HIP_TAP_GROUP_COLOUR_MARGIN) {
				for (size_t g = 0; g < G; ++g) if (!disp[g]) std::memset((uint32_t*)out + g * NCELLS, 0xFF, (size_t)NCELLS * sizeof(uint32_t));
			} else {
				for (size_t k = 0; k < n; ++k) if (grp[k] < 0 || (size_t)grp[k] >= G || !disp[grp[k]]) std::memset((uint32_t*)out + k * NCELLS, 0, (size_t)NCELLS * sizeof(uint32_t));
			}
			return (int64_t)bytes;
		}
		case CIMBAR_HIP_TAP_STITCH_CELLS:
		case CIMBAR_HIP_TAP_STITCH_LINES: {
			if (ctx->stitch_n <= 0) { ctx->err = "tap: the last batch was not a stitched one (cimbar_hip_decode_batch_stitched / _scan_extract_decode_batch_stitched_fmt and their stream forms)"; return CIMBAR_HIP_EINVAL; }
			const size_t pairs = (size_t)ctx->stitch_rows, slots = 2 * pairs, L = (size_t)stitch_lines(ctx->stitch_axis);
			bytes = what == CIMBAR_HIP_TAP_STITCH_LINES ? pairs * L * sizeof(uint16_t) : slots * NCELLS;
			if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
			if (!bytes) return 0;
			if (what == CIMBAR_HIP_TAP_STITCH_LINES) { HIPCHK(hipMemcpy(out, ctx->d_slines, bytes, hipMemcpyDeviceToHost)); return (int64_t)bytes; }
			std::vector<uint8_t> col(bytes);
			std::vector<uint32_t> lv(slots);
			HIPCHK(hipMemcpy(out, ctx->d_ssym, bytes, hipMemcpyDeviceToHost));
			HIPCHK(hipMemcpy(col.data(), ctx->d_scol, bytes, hipMemcpyDeviceToHost));
			HIPCHK(hipMemcpy(lv.data(), ctx->d_slive, sizeof(uint32_t) * slots, hipMemcpyDeviceToHost));
			for (size_t k = 0; k < bytes; ++k) ((uint8_t*)out)[k] = lv[k / NCELLS] ? (uint8_t)((col[k] << 4) | (((uint8_t*)out)[k] & 15u)) : (uint8_t)0;
			return (int64_t)bytes;
		}
		case CIMBAR_HIP_TAP_STITCH_DISTANCE:
		case CIMBAR_HIP_TAP_STITCH_COLOUR_MARGIN: {
			const bool dist = what == CIMBAR_HIP_TAP_STITCH_DISTANCE;
			if (ctx->stitch_n <= 0 || !(ctx->stitch_er_ran & (dist ? 1 : 2))) { ctx->err = "tap: the last batch was not a plain stitched one that ran this retry (cimbar_hip_set_stitch_erasure with the erasure setting on)"; return CIMBAR_HIP_EINVAL; }
			const size_t slots = 2 * (size_t)ctx->stitch_rows, row = (size_t)NCELLS * (dist ? 1 : sizeof(uint32_t));
			bytes = slots * row;
			if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
			std::vector<uint32_t> worked(slots);
			HIPCHK(hipMemcpy(out, dist ? (const void*)ctx->d_sdist.get() : (const void*)ctx->d_smargin.get(), bytes, hipMemcpyDeviceToHost));
			HIPCHK(hipMemcpy(worked.data(), ctx->d_sworked + (dist ? 0 : slots), sizeof(uint32_t) * slots, hipMemcpyDeviceToHost));
			// slots that are not live or lacked nothing: the retry returned at once and computed no confidence
			for (size_t g = 0; g < slots; ++g) if (!worked[g]) std::memset((uint8_t*)out + g * row, 0xFF, row);
			return (int64_t)bytes;
		}
		case CIMBAR_HIP_TAP_STITCH_STRIPS:
		case CIMBAR_HIP_TAP_STITCH_STRIP_LINES: {
			if (ctx->stitch_n <= 0 || ctx->stitch_S <= 1) { ctx->err = "tap: the last batch was not a stitched one with strips above 1 (cimbar_hip_set_stitch_strips)"; return CIMBAR_HIP_EINVAL; }
			const size_t rows = (size_t)ctx->stitch_rows * (size_t)ctx->stitch_S, L = (size_t)stitch_lines(ctx->stitch_axis);
			bytes = what == CIMBAR_HIP_TAP_STITCH_STRIPS ? rows * 4 * sizeof(int32_t) : rows * L * sizeof(uint16_t);
			if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
			if (!bytes) return 0;
			HIPCHK(hipMemcpy(out, what == CIMBAR_HIP_TAP_STITCH_STRIPS ? (const void*)ctx->d_sstrips.get() : (const void*)ctx->d_sstrip_lines.get(), bytes, hipMemcpyDeviceToHost));
			return (int64_t)bytes;
		}
		case CIMBAR_HIP_TAP_STREAM_CARRY_WEIGHTS: {
			// the carried weight rows of slots 0 .. rows - 1, rows = what the buffer holds; every cell of an occupied slot is filled
			if (!ctx->grp_valid || !ctx->gcv_valid || ctx->gcv_stream_n < 0 || !ctx->cstream || !ctx->cstream->weights) { ctx->err = "tap: the last batch was not a stream call with the colour vote on (cimbar_hip_set_stream_colour_vote)"; return CIMBAR_HIP_EINVAL; }
			const size_t row = (size_t)NCELLS * sizeof(uint32_t), rows = out_bytes / row;
			int occupied = 0;
			HIPCHK(hipMemcpy(&occupied, ctx->cstream->words, sizeof(int), hipMemcpyDeviceToHost));
			if (rows > (size_t)occupied) { ctx->err = "tap: more rows than the carry store has occupied slots"; return CIMBAR_HIP_EINVAL; }
			if (rows) HIPCHK(hipMemcpy2D(out, row, ctx->cstream->weights, CS_WEIGHTS * sizeof(uint32_t), row, rows, hipMemcpyDeviceToHost));
			return (int64_t)(rows * row);
		}
#ifdef FLOOD_PROF
		case 100: {   // cycle counters of the flood kernel, per workgroup area (= per frame while the batch fits the grid). k_flood: 10 x u64 (pop,
			          // decode, offers, pushes, #pops, #pushes, max heap, ...); k_flood3: 8 x u64 for the heap wavefront (hand-over, pushes, pop, -, -,
			          // waiting at the barrier, steps) and 8 for the decoding one (hand-over, -, -, window fetch, decode + offers, waiting, steps)
			bytes = n * 128;
			if (out_bytes < bytes) return CIMBAR_HIP_EINVAL;
			HIPCHK(hipDeviceSynchronize());
			for (size_t k = 0; k < n; ++k) HIPCHK(hipMemcpy((uint8_t*)out + k * 128, ctx->flood.heap + k * HEAP_CAP, 128, hipMemcpyDeviceToHost));
			return (int64_t)bytes;
		}
#endif
		default: ctx->err = "tap: unknown selector"; return CIMBAR_HIP_EINVAL;
	}
	if (out_bytes < bytes) { ctx->err = "tap: buffer too small"; return CIMBAR_HIP_EINVAL; }
	HIPCHK(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
	if (what == CIMBAR_HIP_TAP_DRIFT) {
		// frames that took the parallel path never wrote their (all-zero) drift
		std::vector<uint32_t> fl(n);
		HIPCHK(hipMemcpy(fl.data(), cur.d_flood, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
		for (size_t k = 0; k < n; ++k) if (!fl[k]) std::memset((uint8_t*)out + k * NCELLS * 2, 0, (size_t)NCELLS * 2);
	}
	return (int64_t)bytes;
}

int cimbar_hip_enable_timing(cimbar_hip_ctx* ctx, int on)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	ctx->timing = on != 0;
	return 0;
}

int cimbar_hip_stage_times(cimbar_hip_ctx* ctx, const char** names, float* ms, int max)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (ctx->timing && ctx->last_n > 0) {
		// device-output batches do not synchronise inside decode_batch; resolve the events here
		HIPCHK(hipEventSynchronize(ctx->ev[cimbar_hip_ctx::NSTAGE]));
		if (int r = read_stage_times(ctx)) return r;
	}
	int k = 0;
	for (; k < cimbar_hip_ctx::NSTAGE && k < max; ++k) {
		if (names) names[k] = STAGE_NAMES[k];
		if (ms) ms[k] = ctx->stage_ms[k];
	}
	return k;
}


// ---- lens undistortion (undistort.hip.inc) --------------------------------------------------------------------------------------------
namespace {

#pragma clang fp contract(off)
// [assumed-OpenCV] The column table of U2: initUndistortRectifyMap (undistort.simd.hpp) walks each row with running sums, _x = i*ir[1] + ir[2]
// then _x += ir[0] per column, and divides by _w = i*ir[7] + ir[8] (+= ir[6]). For a zero-skew camera ir[1] = ir[3] = ir[6] = ir[7] = 0, so
// _x depends on the column alone and _w is ir[8] everywhere: x_j = _x_j * (1 / ir[8]), summed serially here, once per batch. This restates the
// scalar loop; OpenCV's 64-bit SIMD body instead restarts the sum at every 2 * vlanes columns from lane offsets k * ir[0] -- where its
// dispatch puts those restarts changes the last bit of some x_j, which the float cast of the map hides almost always. A pin against a real
// OpenCV would change this function and nothing else.
void undistort_column_table(const double ir[9], int w, double* xt)
{
	const double winv = 1. / ir[8];
	double _x = 0 * ir[1] + ir[2];
	for (int j = 0; j < w; ++j, _x += ir[0]) xt[j] = _x * winv;
}

// [assumed-OpenCV] lapack.cpp invert() for 3x3 CV_64F with DECOMP_LU: det3, d = 1 / det, cofactors * d -- what Mat::inv() gives
// initUndistortRectifyMap for iR = (newCameraMatrix * R).inv(), R = identity. false: singular.
bool undistort_invert3x3(const double* S, double* t)
{
	double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
	if (d == 0.) return false;
	d = 1. / d;
	t[0] = (S[4] * S[8] - S[5] * S[7]) * d; t[1] = (S[2] * S[7] - S[1] * S[8]) * d; t[2] = (S[1] * S[5] - S[2] * S[4]) * d;
	t[3] = (S[5] * S[6] - S[3] * S[8]) * d; t[4] = (S[0] * S[8] - S[2] * S[6]) * d; t[5] = (S[2] * S[3] - S[0] * S[5]) * d;
	t[6] = (S[3] * S[7] - S[4] * S[6]) * d; t[7] = (S[1] * S[6] - S[0] * S[7]) * d; t[8] = (S[0] * S[4] - S[1] * S[3]) * d;
	return true;
}

// SimpleCameraCalibration's _targetRatio = edge_to_anchor_ratio(1024, 30, 3) (SimpleCameraCalibration.cpp:14-21,38-41): |(512,3)-(512,30)| / |(30,30)-(994,30)|
double undistort_target_ratio() { return std::sqrt(729.0) / std::sqrt(929296.0); }
#pragma clang fp contract(fast)

// The camera of a call: `params` = camera[9] + distortion[5] (k1 k2 p1 p2 k3), or NULL = SimpleCameraCalibration::naive_radial_undistort
// (SimpleCameraCalibration.h:50-58: [w/4, 0, w/2; 0, h/4, h/2; 0, 0, 1] in INTEGER division, distortion (k1, 0, 0, 0), k1 per capture).
// Cameras with skew (camera[1] or camera[3] != 0, or a bottom row other than [0, 0, 1]) and singular ones: EINVAL.
int undistort_setup(cimbar_hip_ctx* ctx, const char* who, const double* params, unsigned width, unsigned height, UndistortParams* P, double ir[9])
{
	double cam[9] = {(double)(int)(width / 4), 0, (double)(int)(width / 2), 0, (double)(int)(height / 4), (double)(int)(height / 2), 0, 0, 1};
	double dist[5] = {0, 0, 0, 0, 0};
	if (params) {
		for (int k = 0; k < 9; ++k) cam[k] = params[k];
		for (int k = 0; k < 5; ++k) dist[k] = params[9 + k];
		for (int k = 0; k < 14; ++k)
			if (!std::isfinite(params[k])) { ctx->err = std::string(who) + ": camera / distortion parameters must be finite"; return CIMBAR_HIP_EINVAL; }
		if (cam[1] != 0. || cam[3] != 0. || cam[6] != 0. || cam[7] != 0. || cam[8] != 1.) {
			ctx->err = std::string(who) + ": only zero-skew cameras [fx, 0, cx; 0, fy, cy; 0, 0, 1] are supported";
			return CIMBAR_HIP_EINVAL;
		}
	}
	if (!undistort_invert3x3(cam, ir)) { ctx->err = std::string(who) + ": the camera matrix is singular"; return CIMBAR_HIP_EINVAL; }
	*P = UndistortParams{cam[0], cam[4], cam[2], cam[5], dist[0], dist[1], dist[2], dist[3], dist[4], ir[4], ir[5], 1. / ir[8]};
	return 0;
}

// captures per group: as many undistorted RGB8 captures as ud_scratch holds (256 MiB: 43 at 1080p), at least one
int undistort_group(const cimbar_hip_ctx* ctx, unsigned width, unsigned height, int n)
{
	const size_t per = (size_t)width * height * 3, fit = ctx->ud_scratch / per;
	return fit < 1 ? 1 : (fit < (size_t)n ? (int)fit : n);
}

// per-capture state of a call of n captures, the column table for `width` columns (the table goes through pinned staging: an async copy must not
// read a pageable temporary), and -- with `group` > 0 -- the image scratch of one group
int undistort_state(cimbar_hip_ctx* ctx, hipStream_t st, int n, const double ir[9], unsigned width, unsigned height, int group)
{
	// (each of these is replaced behind whatever `st` still has in flight that reads it)
	const size_t need = (size_t)width * height * 3 * (size_t)group;
	if ((size_t)n > ctx->d_ud_status.capacity() || width > ctx->d_ud_xt.capacity() || need > ctx->d_ud_img.capacity()) HIPCHK(hipStreamSynchronize(st));
	HIPCHK(ctx->d_ud_ok.reserve((size_t)n));
	HIPCHK(ctx->d_ud_k1.reserve((size_t)n));
	HIPCHK(ctx->d_ud_status.reserve((size_t)n));
	HIPCHK(ctx->ev_ud_xt.create());
	HIPCHK(hipEventSynchronize(ctx->ev_ud_xt));
	HIPCHK(ctx->d_ud_xt.reserve((size_t)width));
	HIPCHK(ctx->h_ud_xt.reserve((size_t)width));
	HIPCHK(ctx->d_ud_img.reserve(need));
	undistort_column_table(ir, (int)width, ctx->h_ud_xt);
	HIPCHK(hipMemcpyAsync(ctx->d_ud_xt, ctx->h_ud_xt, sizeof(double) * width, hipMemcpyHostToDevice, st));
	HIPCHK(hipEventRecord(ctx->ev_ud_xt, st));
	return 0;
}

// U1 for m device-resident captures: X1 + X2 + S1-S3 (enqueue_scan), then k_undistort_calibrate -> d_ok[m], d_k1[m]
int enqueue_undistort_calibrate(cimbar_hip_ctx* ctx, hipStream_t st, const uint8_t* d_in, unsigned width, unsigned height, int fmt, int m, int* d_ok, double* d_k1)
{
	if (int r = extract_state(ctx, m)) return r;
	if (int r = enqueue_scan(ctx, st, d_in, width, height, fmt, m)) return r;
	hipLaunchKernelGGL(k_undistort_calibrate, dim3((m + 63) / 64), dim3(64), 0, st, ctx->d_ex_gray, (int)width, (int)height, ctx->d_ex_thr,
	                   &ctx->d_scan_res[0].status, (int)(sizeof(ScanResult) / sizeof(int)), ctx->d_scan_res[0].corners, (int)(sizeof(ScanResult) / sizeof(float)),
	                   m, undistort_target_ratio(), d_ok, d_k1);
	HIPCHK(hipGetLastError());
	return 0;
}

// U2 for m captures in `fmt` -> m undistorted RGB8 captures at d_out
void launch_undistort(hipStream_t st, int fmt, const uint8_t* d_in, unsigned width, unsigned height, int m, const double* d_xt, const UndistortParams& P,
                      const double* d_k1, const int* d_ok, uint8_t* d_out)
{
	static const int xcd_order = [] { const char* v = std::getenv("CIMBAR_HIP_WARP_ORDER"); return v ? std::atoi(v) : 1; }();
	const dim3 g((width + 63) / 64, (height + 16 * UD_ROWS - 1) / (16 * UD_ROWS), m);
	const int W = (int)width, H = (int)height;
	for_capture_format(fmt, [&](auto F) { hipLaunchKernelGGL((k_undistort<decltype(F)::value>), g, dim3(256), 0, st, d_in, W, H, d_xt, P, d_k1, d_ok, d_out, xcd_order); });
}

}  // namespace

int cimbar_hip_undistort_calibrate_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n, int img_mem,
                                       int* ok, double* k1, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (!ok || !k1) { ctx->err = "undistort_calibrate: null ok / k1"; return CIMBAR_HIP_EINVAL; }
	CaptureIn cap{width, height, format, nullptr}; hipStream_t st;
	if (int r = begin_decode(ctx, "undistort_calibrate", &cap, img, n, "img_mem", img_mem, true, CIMBAR_HIP_MEM_HOST, hip_stream, false, &st)) return r;
	const int fmt = cap.fmt; const size_t cbytes = cap.cbytes;
	UndistortParams P; double ir[9];
	if (int r = undistort_setup(ctx, "undistort_calibrate", nullptr, width, height, &P, ir)) return r;
	const int group = undistort_group(ctx, width, height, n);
	if (int r = undistort_state(ctx, st, n, ir, width, height, 0)) return r;
	const uint8_t* d_in = nullptr;
	if (int r = stage_input(ctx, st, ctx->d_ex_in, img, cbytes * n, img_mem, &d_in)) return r;
	for (int lo = 0; lo < n; lo += group) {
		const int m = n - lo < group ? n - lo : group;
		if (int r = enqueue_undistort_calibrate(ctx, st, d_in + (size_t)lo * cbytes, width, height, fmt, m, ctx->d_ud_ok + lo, ctx->d_ud_k1 + lo)) return r;
	}
	HIPCHK(hipMemcpyAsync(ok, ctx->d_ud_ok, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(k1, ctx->d_ud_k1, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return 0;
}

int cimbar_hip_undistort_batch_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n, int img_mem,
                                   const double* params, uint8_t* out_rgb, int out_mem, int* ok, double* k1_out, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (!out_rgb) { ctx->err = "undistort_batch: null out_rgb"; return CIMBAR_HIP_EINVAL; }
	CaptureIn cap{width, height, format, nullptr}; hipStream_t st;
	if (int r = begin_decode(ctx, "undistort_batch", &cap, img, n, "img_mem", img_mem, true, out_mem, hip_stream, false, &st)) return r;
	const int fmt = cap.fmt; const size_t cbytes = cap.cbytes;
	UndistortParams P; double ir[9];
	if (int r = undistort_setup(ctx, "undistort_batch", params, width, height, &P, ir)) return r;
	const int group = undistort_group(ctx, width, height, n);
	if (int r = undistort_state(ctx, st, n, ir, width, height, out_mem == CIMBAR_HIP_MEM_HOST ? group : 0)) return r;
	const uint8_t* d_in = nullptr;
	if (int r = stage_input(ctx, st, ctx->d_ex_in, img, cbytes * n, img_mem, &d_in)) return r;
	const size_t per = (size_t)width * height * 3;
	if (params) hipLaunchKernelGGL(k_undistort_fill, dim3((n + 63) / 64), dim3(64), 0, st, n, P.k1, ctx->d_ud_ok, ctx->d_ud_k1);
	for (int lo = 0; lo < n; lo += group) {
		const int m = n - lo < group ? n - lo : group;
		if (!params)
			if (int r = enqueue_undistort_calibrate(ctx, st, d_in + (size_t)lo * cbytes, width, height, fmt, m, ctx->d_ud_ok + lo, ctx->d_ud_k1 + lo)) return r;
		uint8_t* d_out = out_mem == CIMBAR_HIP_MEM_DEVICE ? out_rgb + (size_t)lo * per : ctx->d_ud_img;
		launch_undistort(st, fmt, d_in + (size_t)lo * cbytes, width, height, m, ctx->d_ud_xt, P, params ? nullptr : ctx->d_ud_k1 + lo,
		                 params ? nullptr : ctx->d_ud_ok + lo, d_out);
		HIPCHK(hipGetLastError());
		// (the next group's kernels overwrite the scratch only after this copy: same stream)
		if (out_mem == CIMBAR_HIP_MEM_HOST) HIPCHK(hipMemcpyAsync(out_rgb + (size_t)lo * per, d_out, per * m, hipMemcpyDeviceToHost, st));
	}
	const hipMemcpyKind kind = out_mem == CIMBAR_HIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
	if (ok) HIPCHK(hipMemcpyAsync(ok, ctx->d_ud_ok, sizeof(int) * (size_t)n, kind, st));
	if (k1_out) HIPCHK(hipMemcpyAsync(k1_out, ctx->d_ud_k1, sizeof(double) * (size_t)n, kind, st));
	if (out_mem == CIMBAR_HIP_MEM_DEVICE) return 0;
	HIPCHK(hipStreamSynchronize(st));
	return 0;
}

int64_t cimbar_hip_scan_undistort_extract_decode_batch_fmt(cimbar_hip_ctx* ctx, const uint8_t* img, unsigned width, unsigned height, int format, int n,
                                                           int img_mem, int preprocess, int color_correction, uint8_t* chunks, uint32_t* masks, int* status,
                                                           int* undistort_ok, int out_mem, void* hip_stream)
{
	if (!ctx) return CIMBAR_HIP_EINVAL;
	if (!chunks || !masks) { ctx->err = "scan_undistort_extract_decode_batch: null chunks / masks"; return CIMBAR_HIP_EINVAL; }
	CaptureIn cap{width, height, format, nullptr}; hipStream_t st;
	if (int r = begin_decode(ctx, "scan_undistort_extract_decode_batch", &cap, img, n, "img_mem", img_mem, true, out_mem, hip_stream, false, &st)) return r;
	const int fmt = cap.fmt; const size_t cbytes = cap.cbytes;
	UndistortParams P; double ir[9];
	if (int r = undistort_setup(ctx, "scan_undistort_extract_decode_batch", nullptr, width, height, &P, ir)) return r;
	if (int r = ensure_capacity(ctx, n)) return r;
	const int group = undistort_group(ctx, width, height, n);
	if (int r = undistort_state(ctx, st, n, ir, width, height, group)) return r;
	const uint8_t* d_in = nullptr;
	if (int r = stage_input(ctx, st, ctx->d_ex_in, img, cbytes * n, img_mem, &d_in)) return r;
	HIPCHK(ctx->d_ex_frames.reserve((size_t)n * FRAME_RGB));
	// cimbar.cpp:135-146 per capture, a group at a time: calibrate on the raw capture, remap (a failed calibration leaves the image as it was), then
	// Extractor::extract on the result; the deskewed frames of the whole batch then go through ONE decode, as in scan_extract_decode_batch
	for (int lo = 0; lo < n; lo += group) {
		const int m = n - lo < group ? n - lo : group;
		if (int r = enqueue_undistort_calibrate(ctx, st, d_in + (size_t)lo * cbytes, width, height, fmt, m, ctx->d_ud_ok + lo, ctx->d_ud_k1 + lo)) return r;
		launch_undistort(st, fmt, d_in + (size_t)lo * cbytes, width, height, m, ctx->d_ud_xt, P, ctx->d_ud_k1 + lo, ctx->d_ud_ok + lo, ctx->d_ud_img);
		if (int r = enqueue_scan(ctx, st, ctx->d_ud_img, width, height, FMT_RGB, m)) return r;
		if (int r = launch_warp_ctx(ctx, st, FMT_RGB, ctx->d_ud_img, width, height, m, ctx->d_ex_minv, ctx->d_ex_frames + (size_t)lo * FRAME_RGB)) return r;
		HIPCHK(hipMemcpy2DAsync(ctx->d_ud_status + lo, sizeof(int), &ctx->d_scan_res[0].status, sizeof(ScanResult), sizeof(int), (size_t)m, hipMemcpyDeviceToDevice, st));
	}
	uint8_t* d_chunks = out_mem == CIMBAR_HIP_MEM_DEVICE ? chunks : ctx->d_chunks;
	uint32_t* d_masks = out_mem == CIMBAR_HIP_MEM_DEVICE ? masks : ctx->d_masks;
	if (int r = enqueue_source(ctx, st, deskewed_source(ctx, ctx->d_ud_status, 1, preprocess), n, color_correction, d_chunks, d_masks)) return r;
	const hipMemcpyKind kind = out_mem == CIMBAR_HIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
	if (status) HIPCHK(hipMemcpyAsync(status, ctx->d_ud_status, sizeof(int) * (size_t)n, kind, st));
	if (undistort_ok) HIPCHK(hipMemcpyAsync(undistort_ok, ctx->d_ud_ok, sizeof(int) * (size_t)n, kind, st));
	// (finish_batch alone: unlike decode_impl, this call has never read the stage timers, and still does not)
	return finish_batch(ctx, st, n, chunks, masks, d_chunks, d_masks, out_mem, nullptr);
}
