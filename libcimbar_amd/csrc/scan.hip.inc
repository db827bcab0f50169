// scan.hip.inc -- part of cimbar_hip.hip (one translation unit; included inside its anonymous namespace).
// S1-S3: the anchor search of Scanner (src/lib/extractor/Scanner.h:277-405, Scanner.cpp:52-202, ScanState.h:21-104) on the device, then
// Corners / is_granular_scale (Corners.h:45-73) and the destination->source matrix of Deskewer::deskew -- the glue that turns the two image
// passes of extract.hip.inc into Extractor::extract (Extractor.h:29-45) without a round trip to the host.
// ------------------------------------------------------------------------------------------------ anchor search
// The search works on Scanner::_img, the 0/255 output of preprocess_image; test_pixel (Scanner.cpp:52-59, dark mode) is `pixel > 127`,
// i.e. `blurred gray > Otsu threshold`, so the kernels read the blurred image of X1 and the threshold of X2 and never need X3's binary copy.
//   k_scan_stage_rows  a row scan (t1_scan_rows): one wavefront per (capture, row); 64 pixels per load, turned into a bit mask by a ballot
//                      and consumed run by run by the ScanState machine
//   k_scan_confirm     the column / diagonal / 3+3 confirm scans of every row hit, one wavefront per hit (they depend on the image only)
//   k_scan_select / k_scan_final   the ordered remainder per capture (dedupe in hit order, filter, corner order, the bottom-right search's
//                      set-up and verdict): the reference's control flow on wave-uniform values

struct ScanAnchor { int x, xmax, y, ymax; };
__device__ __forceinline__ int sa_xavg(const ScanAnchor& a) { return (a.x + a.xmax) / 2; }
__device__ __forceinline__ int sa_yavg(const ScanAnchor& a) { return (a.y + a.ymax) / 2; }
__device__ __forceinline__ int sa_xrange(const ScanAnchor& a) { return abs(a.x - a.xmax) / 2; }
__device__ __forceinline__ int sa_yrange(const ScanAnchor& a) { return abs(a.y - a.ymax) / 2; }
__device__ __forceinline__ int sa_max_range(const ScanAnchor& a) { const int p = abs(a.x - a.xmax), q = abs(a.y - a.ymax); return p > q ? p : q; }
// Anchor::size (Anchor.h:77-80): pow(dx, 2) + pow(dy, 2) in double, truncated -- exact in integers for these magnitudes
__device__ __forceinline__ unsigned long long sa_size(const ScanAnchor& a)
{
	const long long dx = a.x - a.xmax, dy = a.y - a.ymax;
	return (unsigned long long)(dx * dx + dy * dy);
}
__device__ __forceinline__ void sa_merge(ScanAnchor& a, const ScanAnchor& o)
{
	a.x = min(a.x, o.x); a.xmax = max(a.xmax, o.xmax); a.y = min(a.y, o.y); a.ymax = max(a.ymax, o.ymax);
}
// Anchor::is_mergeable (Anchor.h:87-95)
__device__ __forceinline__ bool sa_mergeable(const ScanAnchor& a, const ScanAnchor& rhs, int max_distance)
{
	if (abs(sa_xavg(a) - sa_xavg(rhs)) > max_distance || abs(sa_yavg(a) - sa_yavg(rhs)) > max_distance) return false;
	const int mr = sa_max_range(a);
	if (mr == 0) return false;
	const int ratio = sa_max_range(rhs) * 10 / mr;
	return ratio > 6 && ratio < 17;
}

// ScanState (ScanState.h:21-104) is a sliding window over RUNS: its state advances at every change of activity, starting with the first
// active pixel; whenever an active run ends (from the third one on) evaluate_state looks at the last five runs -- active, inactive,
// active, inactive, active, lengths t1..t5 -- and pop_state drops the oldest two. So the hits of a scan line are exactly the active runs
// whose five-run window passes the ratio test (:70-97), and a line can be scanned by finding its run boundaries and testing every window
// independently. KIND 114: limits {3, 6} on all four side runs; 122: {1, 3}, {0.5, 1.5}, {0.5, 1.5}, {1, 3}. Returns the pattern's
// length t1 + .. + t5, or -1.
template <int KIND>
__device__ __forceinline__ int scan_window(int t1, int t2, int t3, int t4, int t5)
{
	const int t[4] = {t1, t2, t4, t5};
	const float center = (float)t3;
	bool okp = true;
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		const bool outer = i == 0 || i == 3;
		const float lo = KIND == 114 ? 3.0f : (outer ? 1.0f : 0.5f);
		const float hi = KIND == 114 ? 6.0f : (outer ? 3.0f : 1.5f);
		const float ratio_min = __fdiv_rn(center, (float)(t[i] + 1));
		const float ratio_max = __fdiv_rn(center, (float)(t[i] - 1 > 1 ? t[i] - 1 : 1));
		if (ratio_max < lo || ratio_min > hi) okp = false;
	}
	return okp ? t1 + t2 + t3 + t4 + t5 : -1;
}

#ifdef CIMBAR_SCAN_TINY_LISTS
constexpr int SCAN_ROW_PTS = 1;        // (test build: nearly every capture overflows its row lists and takes the serial slow path)
#else
constexpr int SCAN_ROW_PTS = 48;       // t1 hits kept per scan row (a row of a mode-B capture yields a handful); more -> the capture takes the serial slow path (k_scan_serial)
#endif
constexpr int SCAN_MAX_ROWS = 128;     // rows / skip is < 61 for landscape captures; portrait ones up to ~107 (16:9)
constexpr int SCAN_MAX_CAND = 64;
constexpr int SCAN_MAX_PTS = 256;      // points one column / diagonal / confirm scan or the bottom-right row scan may return

// LDS lists are written by lane 0 and read by every lane: same wavefront, so program order + a wave barrier is enough
__device__ __forceinline__ void scan_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- one scan line, 64 pixels at a time
struct ScanCtx {
	const uint8_t* img;
	int w, h, skip, cutoff, lane;
	uint32_t thr;
	bool overflow;
};

// 64 pixels of a scan line starting at (x0, y0), step (dx, dy): bit k = test_pixel of pixel k (out of the image: inactive)
__device__ __forceinline__ unsigned long long scan_fetch(const ScanCtx& sc, int x0, int y0, int dx, int dy, int count)
{
	const int x = x0 + sc.lane * dx, y = y0 + sc.lane * dy;
	bool active = false;
	if (sc.lane < count && x >= 0 && y >= 0 && x < sc.w && y < sc.h) active = (uint32_t)sc.img[(size_t)y * sc.w + x] > sc.thr;
	return __ballot(active);
}

// one scan line of `total` pixels from (x0, y0) in direction (dx, dy): scan_horizontal / scan_vertical / scan_diagonal (Scanner.h:167-275),
// by one wavefront. Pass 1: 64 pixels per load, a ballot gives their activity mask, the positions where it changes go to `pos` (LDS, in
// order): pos[0] = start of the first active run, pos[1] = its end, ... The flush after the last pixel (process(false), :187-196) ends a
// run that is still active there. Pass 2: one lane per active run k >= 2 tests its five-run window. A hit at line index e (first pixel
// after the pattern, `total` for the flush) of length res spans [e - res, e - 1]; emit(res, e) is called for every hit, in order.
// cap = capacity of pos; more changes than that -> sc.overflow.
template <int KIND, typename EMIT>
__device__ __forceinline__ void scan_line(ScanCtx& sc, int x0, int y0, int dx, int dy, int total, uint16_t* pos, int cap, EMIT emit)
{
	int m = 0;                  // changes found so far
	bool prev = false;          // activity of the pixel before the current chunk
	for (int base = 0; base < total; base += 64) {
		const int cnt = min(64, total - base);
		const unsigned long long mask = scan_fetch(sc, x0 + base * dx, y0 + base * dy, dx, dy, cnt);
		const unsigned long long valid = cnt == 64 ? ~0ull : ((1ull << cnt) - 1ull);
		const unsigned long long chg = (mask ^ ((mask << 1) | (prev ? 1ull : 0ull))) & valid;     // bit k: pixel k differs from pixel k-1
		const int mine = (int)__popcll(chg & ((1ull << sc.lane) - 1ull));
		if (((chg >> sc.lane) & 1ull) && m + mine < cap) pos[m + mine] = (uint16_t)(base + sc.lane);
		m += (int)__popcll(chg);
		prev = (mask >> (cnt - 1)) & 1ull;
	}
	if (prev && sc.lane == 0 && m < cap) pos[m] = (uint16_t)total;
	if (prev) ++m;
	if (m > cap) { sc.overflow = true; m = cap & ~1; }
	scan_sync();
	// runs: active run j = [pos[2j], pos[2j+1]); its window = active runs j-2, j-1, j and the two gaps between them
	const int nact = m / 2;
	for (int j0 = 2; j0 < nact; j0 += 64) {
		const int j = j0 + sc.lane;
		int res = -1, e = 0;
		if (j < nact) {
			const int p0 = pos[2 * j - 4], p1 = pos[2 * j - 3], p2 = pos[2 * j - 2], p3 = pos[2 * j - 1], p4 = pos[2 * j], p5 = pos[2 * j + 1];
			res = scan_window<KIND>(p1 - p0, p2 - p1, p3 - p2, p4 - p3, p5 - p4);
			e = p5;
		}
		unsigned long long hit = __ballot(res > 0);
		while (hit) {
			const int l = (int)__builtin_ctzll(hit);
			hit &= hit - 1;
			emit(__shfl(res, l), __shfl(e, l));
		}
	}
	scan_sync();   // pos is free for the next line
}

struct ScanList { ScanAnchor* v; int n; };   // v points into LDS
struct ScanPos { uint16_t* pos; int cap; };  // the wavefront's run-boundary scratch (LDS)

template <int KIND, int CAP>
__device__ __forceinline__ bool scan_horizontal(ScanCtx& sc, ScanList& pts, int y, int xstart, int xend, ScanPos sp)
{
	if (xstart < 0) xstart = 0;
	if (xend < 0 || xend > sc.w) xend = sc.w;
	const int init = pts.n;
	scan_line<KIND>(sc, xstart, y, 1, 0, max(0, xend - xstart), sp.pos, sp.cap, [&](int res, int k) {
		const int x = xstart + k;
		if (pts.n < CAP) { if (sc.lane == 0) pts.v[pts.n] = ScanAnchor{x - res, x - 1, y, y}; pts.n++; } else sc.overflow = true;
	});
	return init != pts.n;
}
template <int KIND, int CAP>
__device__ __forceinline__ bool scan_vertical(ScanCtx& sc, ScanList& pts, int x, int xmax, int ystart, int yend, ScanPos sp)
{
	if (xmax < 0) xmax = x;
	const int xavg = (x + xmax) / 2;
	if (ystart < 0) ystart = 0;
	if (yend < 0 || yend > sc.h) yend = sc.h;
	const int init = pts.n;
	scan_line<KIND>(sc, xavg, ystart, 0, 1, max(0, yend - ystart), sp.pos, sp.cap, [&](int res, int k) {
		const int y = ystart + k;
		if (pts.n < CAP) { if (sc.lane == 0) pts.v[pts.n] = ScanAnchor{xavg, xavg, y - res, y - 1}; pts.n++; } else sc.overflow = true;
	});
	return init != pts.n;
}
template <int KIND, int CAP>
__device__ __forceinline__ bool scan_diagonal(ScanCtx& sc, ScanList& pts, int xstart, int xend, int ystart, int yend, ScanPos sp)
{
	xend = min(xend, sc.w);
	yend = min(yend, sc.h);
	if (xstart < 0) { const int off = -xstart; xstart += off; ystart += off; }
	if (ystart < 0) { const int off = -ystart; xstart += off; ystart += off; }
	const int init = pts.n;
	const int total = max(0, min(xend - xstart, yend - ystart));
	scan_line<KIND>(sc, xstart, ystart, 1, 1, total, sp.pos, sp.cap, [&](int res, int k) {
		const int x = xstart + k, y = ystart + k;
		if (pts.n < CAP) { if (sc.lane == 0) pts.v[pts.n] = ScanAnchor{x - res, x - 1, y - res, y - 1}; pts.n++; } else sc.overflow = true;
	});
	return init != pts.n;
}

// t4_confirm_scan (Scanner.h:341-389)
template <int KIND, int CAP>
__device__ __forceinline__ bool scan_t4(ScanCtx& sc, ScanAnchor& hint, bool merge_confirms, ScanAnchor* tmp, ScanPos sp)
{
	{
		ScanList cf{tmp, 0};
		const int xstart = hint.x - sa_xrange(hint), xend = hint.xmax + sa_xrange(hint), yavg = sa_yavg(hint);
		for (int dy = -1; dy <= 1; ++dy)
			if (!scan_horizontal<KIND, CAP>(sc, cf, yavg + dy, xstart, xend, sp)) return false;
		scan_sync();
		bool confirm = false;
		for (int k = 0; k < cf.n; ++k) {
			const ScanAnchor co = cf.v[k];
			if (sa_mergeable(co, hint, sc.cutoff)) {
				confirm = true;
				if (!merge_confirms) break;
				sa_merge(hint, co);
			}
		}
		scan_sync();
		if (!confirm) return false;
	}
	{
		ScanList cf{tmp, 0};
		const int ystart = hint.y - sa_yrange(hint), yend = hint.ymax + sa_yrange(hint), xavg = sa_xavg(hint);
		for (int dx = -1; dx <= 1; ++dx)
			if (!scan_vertical<KIND, CAP>(sc, cf, xavg + dx, xavg + dx, ystart, yend, sp)) return false;
		scan_sync();
		bool confirm = false;
		for (int k = 0; k < cf.n; ++k) {
			const ScanAnchor co = cf.v[k];
			if (sa_mergeable(co, hint, sc.cutoff)) {
				confirm = true;
				if (!merge_confirms) break;
				sa_merge(hint, co);
			}
		}
		scan_sync();
		if (!confirm) return false;
	}
	return true;
}

// ---- the search as a pipeline of short kernels. In on_t1_scan (Scanner.h:391-405) only the first step -- "is this hit mergeable with a
// candidate found so far?" -- depends on the hits before it; the column / diagonal / confirm scans that follow (t2 :295-306, t3 :308-339,
// t4 :341-389) look at the image only. So the expensive part is done for ALL hits at once, one wavefront per hit (k_scan_confirm), and a
// cheap ordered pass per capture (k_scan_select / k_scan_final) replays the reference's sequence: dedupe check, then append what the
// hit's scans confirmed. Same result, 30x less time than one wavefront per capture doing everything in order.
constexpr int SCAN_CONFIRM_POS = 1024;   // run boundaries one confirm scan line may have (they are a few hundred pixels long)
constexpr int SCAN_ROW_POS = 4096;       // ... and one full-width row (a 1080p mode-B row has ~400)
constexpr int SCAN_HMAX = 1024;      // hits per capture the confirm stage handles (a 1080p mode-B capture has ~150)
constexpr int SCAN_CONF_MAX = 3;     // confirmed candidates one hit can contribute (its column scan may return more than one pattern)

struct ScanConf { int n; ScanAnchor a[SCAN_CONF_MAX]; };

// exclusive prefix of the per-row hit counts: offs[f][r] = index of row r's first hit in the capture's row-major hit order; offs[f][rows] = total
__global__ __launch_bounds__(64) void k_scan_offsets(const int* __restrict__ nhits, int rows_cap, int row_pts, int* __restrict__ offs, int* __restrict__ overflow)
{
	const int f = blockIdx.x, lane = threadIdx.x;
	int running = 0;
	bool ovf = false;
	for (int base = 0; base < rows_cap; base += 64) {
		const int r = base + lane;
		int c = r < rows_cap ? nhits[(size_t)f * rows_cap + r] : 0;
		if (c > row_pts) { ovf = true; c = row_pts; }
		// inclusive scan over the wave (DPP-free: rows_cap is 128, this runs twice)
		int incl = c;
		for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d); if (lane >= d) incl += o; }
		if (r < rows_cap) offs[(size_t)f * (rows_cap + 1) + r] = running + incl - c;
		running += __shfl(incl, 63);
	}
	if (lane == 0) {
		offs[(size_t)f * (rows_cap + 1) + rows_cap] = running;
		if (__any(ovf) || running > SCAN_HMAX) overflow[f] = 1;
	}
	if (lane != 0 && ovf) overflow[f] = 1;
}

// parameters of one row-scan stage of a capture: rows y0, y0 + skip, ... (count rows), columns [x0, x1)
struct ScanStage { int y0, skip, rows, x0, x1; unsigned cutoff; int found; ScanAnchor a[3]; };

// t2 -> t3 -> t4 for hit h of capture f (row-major order), independent of every other hit
template <int KIND>
__global__ __launch_bounds__(256) void k_scan_confirm(const uint8_t* __restrict__ img, int w, int h, const int* __restrict__ thr,
                                                      const uint32_t* __restrict__ hits, const int* __restrict__ offs, const ScanStage* __restrict__ stage,
                                                      int rows_cap, int row_pts, bool merge_confirms, ScanConf* __restrict__ conf, int* __restrict__ overflow)
{
	__shared__ ScanAnchor s_col[4][64], s_diag[4][64], s_tmp[4][64];
	__shared__ uint16_t s_pos[4][SCAN_CONFIRM_POS];
	const int f = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const ScanPos sp{s_pos[wv], SCAN_CONFIRM_POS};
	const int hidx = blockIdx.x * 4 + wv;
	const int* of = offs + (size_t)f * (rows_cap + 1);
	const int total = min(of[rows_cap], SCAN_HMAX);
	if (hidx >= total) return;
	// which row holds hit hidx: the last row whose offset is <= hidx
	int r = 0;
	for (int base = 0; base < rows_cap; base += 64) {
		const int rr = base + lane;
		const unsigned long long le = __ballot(rr < rows_cap && of[rr] <= hidx);
		if (le) r = base + 63 - (int)__builtin_clzll(le);
	}
	const int k = hidx - of[r];
	const ScanStage sg = stage[f];
	const uint32_t hv = hits[((size_t)f * rows_cap + r) * row_pts + k];
	const int y = sg.y0 + r * sg.skip;
	const ScanAnchor found{(int)(hv & 0xFFFFu), (int)(hv >> 16), y, y};
	ScanCtx sc;
	sc.img = img + (size_t)f * w * h;
	sc.w = w; sc.h = h; sc.lane = lane;
	sc.skip = (h < w ? h : w) / 60;
	sc.cutoff = w / 30;
	sc.thr = (uint32_t)thr[f];
	sc.overflow = false;
	ScanConf out;
	out.n = 0;
	// (the per-wave LDS lists hold 64 entries: a column / diagonal / confirm scan of one anchor-sized stretch returns a handful)
	ScanList col{s_col[wv], 0};
	scan_vertical<KIND, 64>(sc, col, found.x, found.xmax, found.y - 3 * sa_xrange(found), found.ymax + 3 * sa_xrange(found), sp);
	scan_sync();
	for (int q = 0; q < col.n; ++q) {
		const ScanAnchor p = col.v[q];
		ScanList dg{s_diag[wv], 0};
		const int yr = sa_yrange(p);
		if (!scan_diagonal<KIND, 64>(sc, dg, sa_xavg(p) - 2 * yr, sa_xavg(p) + 2 * yr, p.y - yr, p.ymax + yr, sp)) continue;
		scan_sync();
		bool confirm = false;
		ScanAnchor merged = p;
		for (int d = 0; d < dg.n; ++d) {
			const ScanAnchor co = dg.v[d];
			if (sa_mergeable(co, p, sc.cutoff)) { confirm = true; sa_merge(merged, co); }
		}
		scan_sync();
		if (confirm && scan_t4<KIND, 64>(sc, merged, merge_confirms, s_tmp[wv], sp)) {
			if (out.n < SCAN_CONF_MAX) out.a[out.n] = merged; else sc.overflow = true;
			out.n++;
		}
	}
	if (lane == 0) {
		if (out.n > SCAN_CONF_MAX) out.n = SCAN_CONF_MAX;
		conf[(size_t)f * SCAN_HMAX + hidx] = out;
		if (sc.overflow) overflow[f] = 1;
	}
}

// the ordered part of on_t1_scan over a stage's hits: a hit that is mergeable with a candidate found so far contributes nothing, any other
// appends what its scans confirmed. One wavefront (everything is tiny and uniform); returns the number of candidates.
__device__ __forceinline__ int scan_replay(const uint32_t* __restrict__ hits, const int* __restrict__ of, const ScanConf* __restrict__ conf, const ScanStage& sg,
                                           int rows_cap, int row_pts, int cutoff, ScanAnchor* cand, int lane, bool& overflow)
{
	int n = 0;
	const int total = min(of[rows_cap], SCAN_HMAX);
	int r = 0;
	for (int hidx = 0; hidx < total; ++hidx) {
		while (r + 1 <= rows_cap && of[r + 1] <= hidx) ++r;
		const uint32_t hv = hits[((size_t)r) * row_pts + (hidx - of[r])];
		const int y = sg.y0 + r * sg.skip;
		const ScanAnchor found{(int)(hv & 0xFFFFu), (int)(hv >> 16), y, y};
		bool dup = false;
		for (int c = 0; c < n; ++c) if (sa_mergeable(cand[c], found, cutoff)) { dup = true; break; }
		if (dup) continue;
		const ScanConf cf = conf[hidx];
		for (int q = 0; q < cf.n; ++q) {
			if (n < SCAN_MAX_CAND) { if (lane == 0) cand[n] = cf.a[q]; ++n; } else overflow = true;
		}
		scan_sync();
	}
	return n;
}

// scan_primary's tail (filter_candidates, sort_top_to_bottom: Scanner.cpp:79-139) and the set-up of add_bottom_right_corner's row scan (:141-169)
__global__ __launch_bounds__(64) void k_scan_select(const uint32_t* __restrict__ hits, const int* __restrict__ offs, const ScanConf* __restrict__ conf,
                                                    const ScanStage* __restrict__ stage1, int w, int h, ScanStage* __restrict__ stage2, int* __restrict__ overflow)
{
	__shared__ ScanAnchor s_cand[SCAN_MAX_CAND];
	const int f = blockIdx.x, lane = threadIdx.x;
	const int skip0 = (h < w ? h : w) / 60, mcut = w / 30;
	bool ovf = false;
	int ncand = scan_replay(hits + (size_t)f * SCAN_MAX_ROWS * SCAN_ROW_PTS, offs + (size_t)f * (SCAN_MAX_ROWS + 1), conf + (size_t)f * SCAN_HMAX, stage1[f],
	                        SCAN_MAX_ROWS, SCAN_ROW_PTS, mcut, s_cand, lane, ovf);
	scan_sync();
	// filter_candidates: std::sort by size, descending -- an insertion sort for <= 16 elements (stable); lane 0
	unsigned cutoff = 0;
	if (ncand >= 3) {
		if (lane == 0) {
			for (int i = 1; i < ncand; ++i) {
				const ScanAnchor key = s_cand[i];
				int j = i - 1;
				while (j >= 0 && sa_size(key) > sa_size(s_cand[j])) { s_cand[j + 1] = s_cand[j]; --j; }
				s_cand[j + 1] = key;
			}
		}
		scan_sync();
		unsigned long long cs = 0;
		for (int i = 0; i < 3; ++i) cs += sa_size(s_cand[i]);
		cutoff = (unsigned)cs;
		cutoff /= 8;
		int i = 0;
		for (; i < ncand; ++i) if (sa_size(s_cand[i]) < cutoff) break;
		if (i > 3) i = 3;
		if (i < ncand) ncand = i;
	}
	ScanStage st{};
	st.found = ncand;
	st.cutoff = cutoff;
	if (ncand >= 3) {
		// sort_top_to_bottom
		const ScanAnchor c[3] = {s_cand[0], s_cand[1], s_cand[2]};
		int cx[3], cy[3];
		for (int i = 0; i < 3; ++i) { cx[i] = sa_xavg(c[i]); cy[i] = sa_yavg(c[i]); }
		const int ex[3] = {cx[1] - cx[2], cx[2] - cx[0], cx[0] - cx[1]}, ey[3] = {cy[1] - cy[2], cy[2] - cy[0], cy[0] - cy[1]};
		int tl = 0, maxd = 0;
		for (int i = 0; i < 3; ++i) { const int d = ex[i] * ex[i] + ey[i] * ey[i]; if (d > maxd) { tl = i; maxd = d; } }
		const int dep = tl - 1 < 0 ? 2 : tl - 1, inc = tl + 1 >= 3 ? 0 : tl + 1;
		const int ix = -ey[inc], iy = ex[inc];
		const int ox = ex[dep] - ix, oy = ey[dep] - iy;
		int tr, bl;
		if (ox * ox + oy * oy < ex[dep] * ex[dep] + ey[dep] * ey[dep]) { tr = inc; bl = dep; }
		else { tr = dep; bl = inc; }
		st.a[0] = c[tl]; st.a[1] = c[tr]; st.a[2] = c[bl];
		st.found = 3;
	} else {
		for (int i = 0; i < ncand && i < 3; ++i) st.a[i] = s_cand[i];
	}
	st.rows = 0;
	if (st.found == 3 && cutoff != 0) {
		// add_bottom_right_corner: where the fourth, smaller anchor should be, and the window its finer row scan covers
		const ScanAnchor a0 = st.a[0], a1 = st.a[1], a2 = st.a[2];
		const int mr0 = sa_max_range(a0), mr1 = sa_max_range(a1), mr2 = sa_max_range(a2);
		const double top_scalar = (double)mr2 / (double)max(mr1, mr0);
		const int tex = (int)((double)(sa_xavg(a1) - sa_xavg(a0)) * top_scalar), tey = (int)((double)(sa_yavg(a1) - sa_yavg(a0)) * top_scalar);
		const int g1x = sa_xavg(a2) + tex, g1y = sa_yavg(a2) + tey;
		const double left_scalar = (double)mr1 / (double)max(mr2, mr0);
		const int lex = (int)((double)(sa_xavg(a2) - sa_xavg(a0)) * left_scalar), ley = (int)((double)(sa_yavg(a2) - sa_yavg(a0)) * left_scalar);
		const int g2x = sa_xavg(a1) + lex, g2y = sa_yavg(a1) + ley;
		const int ccx = (g1x + g2x) / 2, ccy = (g1y + g2y) / 2;
		const int range = (int)((float)max(mr0, max(mr1, mr2)) * 2.0f);
		// t1_scan_rows(fun, skip, ystart, yend, xstart, xend) (Scanner.h:277-293)
		int skip = skip0 / 2;
		if (skip <= 0) skip = skip0;
		int y = ccy - range, yend = ccy + range;
		if (y < 0) y = skip;
		if (yend < 0 || yend > h) yend = h;
		int x0 = ccx - range, x1 = ccx + range;
		if (x0 < 0) x0 = 0;
		if (x1 < 0 || x1 > w) x1 = w;
		st.y0 = y; st.skip = skip; st.x0 = x0; st.x1 = x1;
		st.rows = (skip > 0 && yend > y) ? (yend - y + skip - 1) / skip : 0;
		if (st.rows > SCAN_MAX_ROWS) { st.rows = SCAN_MAX_ROWS; ovf = true; }
	}
	if (lane == 0) {
		stage2[f] = st;
		if (ovf) overflow[f] = 1;
	}
}

// the row scan of a stage: one wavefront per (capture, row), pattern KIND, columns [x0, x1) -- t1_scan_rows / scan_horizontal
template <int KIND>
__global__ __launch_bounds__(256) void k_scan_stage_rows(const uint8_t* __restrict__ img, int w, int h, const int* __restrict__ thr,
                                                         const ScanStage* __restrict__ stage, int n, uint32_t* __restrict__ hits, int* __restrict__ nhits)
{
	__shared__ uint16_t s_pos[4][SCAN_ROW_POS];
	const int gid = blockIdx.x * 4 + (threadIdx.x >> 6);
	const int f = gid / SCAN_MAX_ROWS, r = gid % SCAN_MAX_ROWS;
	if (f >= n) return;
	const ScanStage sg = stage[f];
	int cnt = 0;
	bool sc_overflow = false;
	uint32_t* out = hits + ((size_t)f * SCAN_MAX_ROWS + r) * SCAN_ROW_PTS;
	if (r < sg.rows) {
		ScanCtx sc;
		sc.img = img + (size_t)f * w * h;
		sc.w = w; sc.h = h; sc.lane = threadIdx.x & 63; sc.skip = 0; sc.cutoff = 0; sc.overflow = false;
		sc.thr = (uint32_t)thr[f];
		const int y = sg.y0 + r * sg.skip;
		scan_line<KIND>(sc, sg.x0, y, 1, 0, max(0, sg.x1 - sg.x0), s_pos[threadIdx.x >> 6], SCAN_ROW_POS, [&](int res, int k) {
			const int x = sg.x0 + k;
			if (cnt < SCAN_ROW_PTS && sc.lane == 0) out[cnt] = (uint32_t)(x - res) | ((uint32_t)(x - 1) << 16);
			++cnt;
		});
		sc_overflow = sc.overflow;
	}
	if ((threadIdx.x & 63) == 0) nhits[(size_t)f * SCAN_MAX_ROWS + r] = sc_overflow ? SCAN_ROW_PTS + 1 : cnt;   // (an overflowing row reads as too many hits)
}

// the primary stage's parameters: every row skip, 2 skip, ... over the full width (Scanner.h:277-293 defaults)
__global__ __launch_bounds__(64) void k_scan_stage1(int w, int h, int n, ScanStage* __restrict__ stage, int* __restrict__ overflow)
{
	const int f = blockIdx.x * 64 + threadIdx.x;
	if (f >= n) return;
	ScanStage st{};
	const int skip = (h < w ? h : w) / 60;
	st.y0 = skip; st.skip = skip; st.x0 = 0; st.x1 = w;
	st.rows = skip > 0 ? (h - 1) / skip : 0;
	overflow[f] = 0;
	if (f == 0) overflow[n] = 0;                       // the slow path's scratch-slot counter (k_scan_serial)
	if (st.rows > SCAN_MAX_ROWS) { st.rows = SCAN_MAX_ROWS; overflow[f] = 1; }
	stage[f] = st;
}

// result[f] = {status, found, corners[8]}: status 0 FAILURE / 1 SUCCESS / 2 NEEDS_SHARPEN (Extractor.h:18-20), -1 = a fixed-size list
// of these kernels overflowed (the capture is then treated as a failure); corners = Corners::all() (top-left, top-right, bottom-left,
// bottom-right; x, y) as floats
struct ScanResult { int status, found; float corners[8]; int anchors[16]; };

// add_bottom_right_corner's tail (Scanner.cpp:170-181): the first confirmed 1:2:2:2:1 candidate larger than the cutoff; then Corners and
// Extractor::extract's verdict (Extractor.h:33-44)
__global__ __launch_bounds__(64) void k_scan_final(const uint32_t* __restrict__ hits2, const int* __restrict__ offs2, const ScanConf* __restrict__ conf2,
                                                   const ScanStage* __restrict__ stage2, int w, const int* __restrict__ overflow,
                                                   ScanResult* __restrict__ results)
{
	__shared__ ScanAnchor s_c2[SCAN_MAX_CAND];
	const int f = blockIdx.x, lane = threadIdx.x;
	const ScanStage sg = stage2[f];
	bool ovf = overflow[f] != 0;
	int found = sg.found;
	ScanAnchor a3{};
	if (sg.rows > 0) {
		const int n2 = scan_replay(hits2 + (size_t)f * SCAN_MAX_ROWS * SCAN_ROW_PTS, offs2 + (size_t)f * (SCAN_MAX_ROWS + 1), conf2 + (size_t)f * SCAN_HMAX, sg,
		                           SCAN_MAX_ROWS, SCAN_ROW_PTS, w / 30, s_c2, lane, ovf);
		scan_sync();
		for (int k = 0; k < n2; ++k)
			if (sa_size(s_c2[k]) > sg.cutoff) { a3 = s_c2[k]; found = 4; break; }
	}
	if (lane == 0) {
		ScanResult r;
		r.found = found;
		const ScanAnchor an[4] = {sg.a[0], sg.a[1], sg.a[2], a3};
		int cx[4], cy[4];
		for (int i = 0; i < 4; ++i) {
			cx[i] = sa_xavg(an[i]); cy[i] = sa_yavg(an[i]);
			r.corners[2 * i] = (float)cx[i]; r.corners[2 * i + 1] = (float)cy[i];
			r.anchors[4 * i] = an[i].x; r.anchors[4 * i + 1] = an[i].xmax; r.anchors[4 * i + 2] = an[i].y; r.anchors[4 * i + 3] = an[i].ymax;
		}
		int status = 0;
		if (ovf) status = -1;
		else if (found >= 4) {
			// Corners::is_granular_scale({1024, 1024}) (Corners.h:55-73): every edge longer than the output in x or in y
			const int e[4][2] = {{0, 1}, {1, 3}, {3, 2}, {2, 0}};
			bool granular = true;
			for (int k = 0; k < 4; ++k) {
				const int a = e[k][0], b = e[k][1];
				if (!(abs(cx[a] - cx[b]) > IMG_W || abs(cy[a] - cy[b]) > IMG_H)) granular = false;
			}
			status = granular ? 1 : 2;
		}
		r.status = status;
		results[f] = r;
	}
}

// a capture the extractor gave up on (status <= 0) delivers nothing: cimbar.cpp:141-146 skips the frame. One workgroup per frame.
__global__ __launch_bounds__(256) void k_mask_failed(const int* __restrict__ status, int stride, int n, uint32_t* __restrict__ masks,
                                                     uint8_t* __restrict__ chunks)
{
	const int f = blockIdx.x;
	if (status[(size_t)f * stride] > 0) return;
	if (threadIdx.x == 0) masks[f] = 0;
	for (int k = threadIdx.x; k < FRAME_BYTES; k += 256) chunks[(size_t)f * FRAME_BYTES + k] = 0;
}

// ---- the slow path: Scanner::scan by ONE lane, with lists in global memory ------------------------------------------------------------
// The kernels above keep their work lists in fixed-size LDS / register arrays (a mode-B capture needs a few dozen entries); a capture with
// hundreds of anchor-like patterns on one scan line overflows one of them and used to be reported as status -1. Such a capture now goes
// through k_scan_serial: the reference's own control flow (Scanner.cpp:79-202, Scanner.h:167-405, ScanState.h:21-104), statement for
// statement, on one lane per capture, its vectors in a scratch area of global memory (SCAN_SERIAL_CAP entries per list; a capture that
// overflows THOSE -- tens of thousands of patterns -- keeps status -1). Slow (a 1080p capture: milliseconds) and only ever taken by captures
// the fast kernels gave up on; -DCIMBAR_SCAN_TINY_LISTS (the test build) shrinks the fast kernels' lists so that ordinary captures take it.
constexpr int SCAN_SERIAL_CAP = 16384, SCAN_SERIAL_SLOTS = 16;   // list capacity; captures per batch that can take the slow path (1.5 MB of scratch each)
struct SerialList { ScanAnchor* v; int n; bool ovf; };
__device__ __forceinline__ void sl_push(SerialList& l, const ScanAnchor& a) { if (l.n < SCAN_SERIAL_CAP) l.v[l.n++] = a; else l.ovf = true; }

struct SerialState { int state, nt; int tally[8]; };
__device__ __forceinline__ void ss_init(SerialState& s) { s.state = 0; s.nt = 1; s.tally[0] = 0; }
// ScanState::process (ScanState.h:21-60, evaluate_state :70-97, pop_state :63-68)
template <int KIND>
__device__ __forceinline__ int ss_process(SerialState& s, bool active)
{
	const bool even = s.state == 0 || s.state == 2 || s.state == 4;
	const bool odd = s.state == 1 || s.state == 3 || s.state == 5;
	if ((even && active) || (odd && !active)) {
		s.state += 1;
		s.tally[s.nt++] = 1;
		if (s.state == 6) {
			int res = -1;
			bool okp = true;
			for (int i = 1; i <= 5; ++i) if (s.tally[i] == 0) okp = false;
			if (okp) res = scan_window<KIND>(s.tally[1], s.tally[2], s.tally[3], s.tally[4], s.tally[5]);
			s.state -= 2;
			for (int i = 0; i + 2 < s.nt; ++i) s.tally[i] = s.tally[i + 2];
			s.nt -= 2;
			return res;
		}
		return -1;
	}
	if (odd && active) s.tally[s.nt - 1] += 1;
	if (!active && (s.state == 2 || s.state == 4)) s.tally[s.nt - 1] += 1;
	return -1;
}

struct SerialScanner { const uint8_t* img; int w, h, skip, cutoff; uint32_t thr; };
__device__ __forceinline__ bool sr_pixel(const SerialScanner& sc, int x, int y)
{
	if (x < 0 || y < 0 || x >= sc.w || y >= sc.h) return false;       // (the reference reads out of bounds here; "inactive", like the fast kernels)
	return (uint32_t)sc.img[(size_t)y * sc.w + x] > sc.thr;
}
template <int KIND>
__device__ bool sr_horizontal(const SerialScanner& sc, SerialList& pts, int y, int xstart, int xend)      // Scanner.h:167-197
{
	if (xstart < 0) xstart = 0;
	if (xend < 0 || xend > sc.w) xend = sc.w;
	const int init = pts.n;
	SerialState st;
	ss_init(st);
	for (int x = xstart; x < xend; ++x) {
		const int res = ss_process<KIND>(st, sr_pixel(sc, x, y));
		if (res > 0) sl_push(pts, ScanAnchor{x - res, x - 1, y, y});
	}
	const int res = ss_process<KIND>(st, false);
	if (res > 0) sl_push(pts, ScanAnchor{xend - res, xend - 1, y, y});
	return init != pts.n;
}
template <int KIND>
__device__ bool sr_vertical(const SerialScanner& sc, SerialList& pts, int x, int xmax, int ystart, int yend)   // Scanner.h:199-233
{
	if (xmax < 0) xmax = x;
	const int xavg = (x + xmax) / 2;
	if (ystart < 0) ystart = 0;
	if (yend < 0 || yend > sc.h) yend = sc.h;
	const int init = pts.n;
	SerialState st;
	ss_init(st);
	for (int y = ystart; y < yend; ++y) {
		const int res = ss_process<KIND>(st, sr_pixel(sc, xavg, y));
		if (res > 0) sl_push(pts, ScanAnchor{xavg, xavg, y - res, y - 1});
	}
	const int res = ss_process<KIND>(st, false);
	if (res > 0) sl_push(pts, ScanAnchor{xavg, xavg, yend - res, yend - 1});
	return init != pts.n;
}
template <int KIND>
__device__ bool sr_diagonal(const SerialScanner& sc, SerialList& pts, int xstart, int xend, int ystart, int yend)   // Scanner.h:235-275
{
	if (xend > sc.w) xend = sc.w;
	if (yend > sc.h) yend = sc.h;
	if (xstart < 0) { const int off = -xstart; xstart += off; ystart += off; }
	if (ystart < 0) { const int off = -ystart; xstart += off; ystart += off; }
	const int init = pts.n;
	SerialState st;
	ss_init(st);
	int x = xstart, y = ystart;
	for (; x < xend && y < yend; ++x, ++y) {
		const int res = ss_process<KIND>(st, sr_pixel(sc, x, y));
		if (res > 0) sl_push(pts, ScanAnchor{x - res, x - 1, y - res, y - 1});
	}
	const int res = ss_process<KIND>(st, false);
	if (res > 0) sl_push(pts, ScanAnchor{x - res, x - 1, y - res, y - 1});
	return init != pts.n;
}
// t4_confirm_scan (Scanner.h:341-389); `tmp` is scratch
template <int KIND>
__device__ bool sr_confirm(const SerialScanner& sc, ScanAnchor& hint, bool merge_confirms, SerialList& tmp)
{
	{
		tmp.n = 0;
		const int xstart = hint.x - sa_xrange(hint), xend = hint.xmax + sa_xrange(hint), yavg = sa_yavg(hint);
		for (int dy = -1; dy <= 1; ++dy)
			if (!sr_horizontal<KIND>(sc, tmp, yavg + dy, xstart, xend)) return false;
		bool confirm = false;
		for (int k = 0; k < tmp.n; ++k)
			if (sa_mergeable(tmp.v[k], hint, sc.cutoff)) {
				confirm = true;
				if (!merge_confirms) break;
				sa_merge(hint, tmp.v[k]);
			}
		if (!confirm) return false;
	}
	{
		tmp.n = 0;
		const int ystart = hint.y - sa_yrange(hint), yend = hint.ymax + sa_yrange(hint), xavg = sa_xavg(hint);
		for (int dx = -1; dx <= 1; ++dx)
			if (!sr_vertical<KIND>(sc, tmp, xavg + dx, xavg + dx, ystart, yend)) return false;
		bool confirm = false;
		for (int k = 0; k < tmp.n; ++k)
			if (sa_mergeable(tmp.v[k], hint, sc.cutoff)) {
				confirm = true;
				if (!merge_confirms) break;
				sa_merge(hint, tmp.v[k]);
			}
		if (!confirm) return false;
	}
	return true;
}
// t1_scan_rows (Scanner.h:277-293) + on_t1_scan (:391-405): t2 column -> t3 diagonal -> t4 confirm
template <int KIND>
__device__ void sr_rows(const SerialScanner& sc, SerialList& cand, bool merge_confirms, int skip, int y, int yend, int xstart, int xend,
                        SerialList& pts, SerialList& col, SerialList& dg, SerialList& tmp)
{
	if (skip <= 0) skip = sc.skip;
	if (y < 0) y = skip;
	if (yend < 0 || yend > sc.h) yend = sc.h;
	pts.n = 0;
	if (skip <= 0) return;                                           // (an image under 60 px: Scanner's loop would not advance; no capture is that small)
	for (; y < yend; y += skip) sr_horizontal<KIND>(sc, pts, y, xstart, xend);
	for (int k = 0; k < pts.n; ++k) {
		const ScanAnchor found = pts.v[k];
		bool dup = false;
		for (int c = 0; c < cand.n; ++c) if (sa_mergeable(cand.v[c], found, sc.cutoff)) { dup = true; break; }
		if (dup) continue;
		col.n = 0;
		sr_vertical<KIND>(sc, col, found.x, found.xmax, found.y - 3 * sa_xrange(found), found.ymax + 3 * sa_xrange(found));
		for (int q = 0; q < col.n; ++q) {
			const ScanAnchor p = col.v[q];
			dg.n = 0;
			const int yr = sa_yrange(p);
			if (sr_diagonal<KIND>(sc, dg, sa_xavg(p) - 2 * yr, sa_xavg(p) + 2 * yr, p.y - yr, p.ymax + yr)) {
				bool confirm = false;
				ScanAnchor merged = p;
				for (int d = 0; d < dg.n; ++d)
					if (sa_mergeable(dg.v[d], p, sc.cutoff)) { confirm = true; sa_merge(merged, dg.v[d]); }
				if (confirm && sr_confirm<KIND>(sc, merged, merge_confirms, tmp)) sl_push(cand, merged);
			}
		}
	}
}

// One lane per capture whose fast search overflowed (results[f].status == -1); overwrites results[f]. scratch: SCAN_SERIAL_SLOTS x 6 lists of
// SCAN_SERIAL_CAP anchors, handed out through *slot_counter (zeroed by k_scan_stage1); grid = captures, a workgroup whose capture did not
// overflow returns at once.
__global__ __launch_bounds__(64) void k_scan_serial(const uint8_t* __restrict__ gray, int w, int h, const int* __restrict__ thr, ScanAnchor* __restrict__ scratch,
                                                    int* __restrict__ slot_counter, int* __restrict__ overflow, ScanResult* __restrict__ results)
{
	const int f = blockIdx.x;
	if (threadIdx.x != 0 || results[f].status != -1) return;
	overflow[f] = 1;                                                    // (k_scan_final's own lists overflow without a flag: CIMBAR_HIP_TAP_SCAN_PATH reads this one)
	const int slot = atomicAdd(slot_counter, 1);
	if (slot >= SCAN_SERIAL_SLOTS) return;                              // more overflowed captures in one batch than there is scratch for: they keep status -1
	ScanAnchor* base = scratch + (size_t)slot * 6 * SCAN_SERIAL_CAP;
	SerialList cand{base, 0, false}, pts{base + SCAN_SERIAL_CAP, 0, false}, col{base + 2 * SCAN_SERIAL_CAP, 0, false},
	           dg{base + 3 * SCAN_SERIAL_CAP, 0, false}, tmp{base + 4 * SCAN_SERIAL_CAP, 0, false}, c2{base + 5 * SCAN_SERIAL_CAP, 0, false};
	const SerialScanner sc{gray + (size_t)f * w * h, w, h, (h < w ? h : w) / 60, w / 30, (uint32_t)thr[f]};
	sr_rows<114>(sc, cand, true, -1, -1, -1, -1, -1, pts, col, dg, tmp);      // scan_primary (Scanner.cpp:171-181)
	// filter_candidates (Scanner.cpp:79-103): std::sort by size, descending. NOT stable for more than 16 elements in libstdc++ (introsort);
	// the insertion sort below is what it does for <= 16 and a stable order beyond -- anchors of equal size in a list that long: see DESIGN.md
	unsigned cutoff = 0;
	int ncand = cand.n;
	if (ncand >= 3) {
		for (int i = 1; i < ncand; ++i) {
			const ScanAnchor key = cand.v[i];
			int j = i - 1;
			while (j >= 0 && sa_size(key) > sa_size(cand.v[j])) { cand.v[j + 1] = cand.v[j]; --j; }
			cand.v[j + 1] = key;
		}
		unsigned long long cs = 0;
		for (int i = 0; i < 3; ++i) cs += sa_size(cand.v[i]);
		cutoff = (unsigned)cs;
		cutoff /= 8;
		int i = 0;
		for (; i < ncand; ++i) if (sa_size(cand.v[i]) < cutoff) break;
		if (i > 3) i = 3;
		if (i < ncand) ncand = i;
	}
	ScanAnchor an[4] = {};
	int found = ncand < 3 ? ncand : 3;
	for (int i = 0; i < found; ++i) an[i] = cand.v[i];
	if (ncand >= 3) {
		// sort_top_to_bottom (Scanner.cpp:105-139)
		const ScanAnchor c[3] = {cand.v[0], cand.v[1], cand.v[2]};
		int cx[3], cy[3];
		for (int i = 0; i < 3; ++i) { cx[i] = sa_xavg(c[i]); cy[i] = sa_yavg(c[i]); }
		const int ex[3] = {cx[1] - cx[2], cx[2] - cx[0], cx[0] - cx[1]}, ey[3] = {cy[1] - cy[2], cy[2] - cy[0], cy[0] - cy[1]};
		int tl = 0, maxd = 0;
		for (int i = 0; i < 3; ++i) { const int d = ex[i] * ex[i] + ey[i] * ey[i]; if (d > maxd) { tl = i; maxd = d; } }
		const int dep = tl - 1 < 0 ? 2 : tl - 1, inc = tl + 1 >= 3 ? 0 : tl + 1;
		const int ix = -ey[inc], iy = ex[inc];
		const int ox = ex[dep] - ix, oy = ey[dep] - iy;
		int tr, bl;
		if (ox * ox + oy * oy < ex[dep] * ex[dep] + ey[dep] * ey[dep]) { tr = inc; bl = dep; }
		else { tr = dep; bl = inc; }
		an[0] = c[tl]; an[1] = c[tr]; an[2] = c[bl];
		found = 3;
		if (cutoff != 0) {
			// add_bottom_right_corner (Scanner.cpp:141-181)
			const int mr0 = sa_max_range(an[0]), mr1 = sa_max_range(an[1]), mr2 = sa_max_range(an[2]);
			const double top_scalar = (double)mr2 / (double)max(mr1, mr0);
			const int tex = (int)((double)(sa_xavg(an[1]) - sa_xavg(an[0])) * top_scalar), tey = (int)((double)(sa_yavg(an[1]) - sa_yavg(an[0])) * top_scalar);
			const int g1x = sa_xavg(an[2]) + tex, g1y = sa_yavg(an[2]) + tey;
			const double left_scalar = (double)mr1 / (double)max(mr2, mr0);
			const int lex = (int)((double)(sa_xavg(an[2]) - sa_xavg(an[0])) * left_scalar), ley = (int)((double)(sa_yavg(an[2]) - sa_yavg(an[0])) * left_scalar);
			const int g2x = sa_xavg(an[1]) + lex, g2y = sa_yavg(an[1]) + ley;
			const int ccx = (g1x + g2x) / 2, ccy = (g1y + g2y) / 2;
			const int range = (int)((float)max(mr0, max(mr1, mr2)) * 2.0f);
			sr_rows<122>(sc, c2, false, sc.skip / 2, ccy - range, ccy + range, ccx - range, ccx + range, pts, col, dg, tmp);
			for (int k = 0; k < c2.n; ++k)
				if (sa_size(c2.v[k]) > cutoff) { an[3] = c2.v[k]; found = 4; break; }
		}
	}
	ScanResult r;
	r.found = found;
	int cx[4], cy[4];
	for (int i = 0; i < 4; ++i) {
		cx[i] = sa_xavg(an[i]); cy[i] = sa_yavg(an[i]);
		r.corners[2 * i] = (float)cx[i]; r.corners[2 * i + 1] = (float)cy[i];
		r.anchors[4 * i] = an[i].x; r.anchors[4 * i + 1] = an[i].xmax; r.anchors[4 * i + 2] = an[i].y; r.anchors[4 * i + 3] = an[i].ymax;
	}
	int status = 0;
	if (cand.ovf || pts.ovf || col.ovf || dg.ovf || tmp.ovf || c2.ovf) status = -1;
	else if (found >= 4) {
		const int e[4][2] = {{0, 1}, {1, 3}, {3, 2}, {2, 0}};
		bool granular = true;
		for (int k = 0; k < 4; ++k) {
			const int a = e[k][0], b = e[k][1];
			if (!(abs(cx[a] - cx[b]) > IMG_W || abs(cy[a] - cy[b]) > IMG_H)) granular = false;
		}
		status = granular ? 1 : 2;
	}
	r.status = status;
	results[f] = r;
}
