// chainplan.hip.inc -- the launch plan of one decode chain: what enqueue() (host.hip.inc) decides before it launches anything, as plain
// arithmetic over plain values. No HIP, no context, no allocation: g++ compiles this file on its own (tools/chain_plan_shim.cpp), and
// tests/test_chain_plan.py holds it against tests/flood_launch_model.py on a CPU. Nothing here depends on the geometry, so cimbar_hip.hip
// includes it once, in front of the per-mode copies.
//
// The rule. A batch runs as ONE chain on the caller's stream, as one chain on the stream of a pipelined SET, or SPLIT into tail_parts parts
// that alternate between the caller's stream and the context's second one. Chains that may be in flight together -- the `ways`: the sets of
// the pipeline, the two streams of a split batch -- each get a slot k: their own share of the flood kernels' spill areas and of
// k_flood_wave's work queues, and their own frame-counter pair.
#include <cstdint>

namespace {

// ---- launch constants
// k_flood3's instances (k2b_flood.hip.inc): HEAP_LDS slots in LDS = three workgroups per CU, 768 frames resident; HEAP_LDS4 = four per CU,
// 1024 resident; the dense one eight per CU, FLOOD_DENSE_PER workgroups (and spill areas) per ordinary one
constexpr int FLOOD_GRID3 = 768, FLOOD_GRID = 1024;
constexpr int FLOOD_DENSE_PER = 2;
constexpr int FW_GRID = 512;             // k_flood_wave (k2c_floodwave.hip.inc): 75 KiB of LDS per workgroup, two per CU
constexpr int FLOOD_COUNTERS = 8;        // FloodScratch::next: pairs (frames handed out, workgroups that have left), one per slot
constexpr int FLOOD_LAUNCH_MAX = 16;     // exact-replay launches CIMBAR_HIP_TAP_FLOOD_LAUNCH keeps of one call
constexpr int CHAIN_PARTS_MAX = 8;       // parts of a split batch (CIMBAR_HIP_TAIL_PARTS)

// what enqueue() reads to decide
struct ChainPlanIn {
	int n = 0;                                   // frames
	bool pipe = false, no_split = false, symbols_only = false;   // ChainArgs
	bool timed = false;                          // stage timing is on (and the batch is not pipelined): measured in the single-stream order
	bool have_flagged = false;                   // the context has the pinned words k_count_flagged reports into ...
	uint32_t flagged[3] = {0, 0, 0};             // ... and what they said when the call began: [0] frames that left the parallel path, [1] frames
	                                             // of that batch, [2] frames the exact replay had to take
	int tail_split = 1, tail_parts = 2;
	int pipe_depth = 3, pipe_set = 0;
	int flood_dense = -1, flood_dense_grid = FLOOD_DENSE_PER * FLOOD_GRID;
	int flood_wave = 1, flood_verify = 0, wave_adapt = 1;
	bool wave_ran = false; int wave_skip_left = 0;   // the wave scheduler's state
	bool relaxed = false, relaxed_fallback = false;  // the relaxed flood is on; ... with its exact fallback
};

// the shares of one slot
struct ChainLane {
	int areas, area0;       // spill areas a flood launch may use, and the first of them
	int wareas, warea0;     // the same of k_flood_wave's work queues
	int counter;            // its counter pair
};
struct ChainPart { int first, count, lane; };
struct ExactLaunch { int instance, grid; bool hand_out; };   // k_flood3's instance 3 / 4 / 8; hand_out: fewer workgroups than frames

struct ChainPlan {
	bool split = false;          // tail_parts parts on two streams
	bool counted = false;        // the batch ends with k_count_flagged
	bool run_wave = false;       // k_flood_wave runs in front of the exact replay
	bool stop_at_mid = false;    // symbols_only; only a single chain stops
	bool wave_ran = false; int wave_skip_left = 0;   // the scheduler's next state
	// which exact replays a part launches, in this order (CIMBAR_HIP_TAP_FLOOD_LAUNCH's flags 0, 1, 2): of the batch's own flags, of what
	// k_flood_wave certified (CIMBAR_HIP_FLOOD_VERIFY), of what the relaxed flood's RS check sent back
	bool exact_batch = false, exact_verify = false, exact_fallback = false;
	int nparts = 1;
	ChainPart part[CHAIN_PARTS_MAX] = {};   // in issue order; a chain that is not split is part 0 on lane 0
	ChainLane lane[2] = {};      // the caller's stream (or the pipelined set's), the context's second stream
	int flood_dense = -1, flood_dense_grid = 0;
	int flood_top = 0;           // spill areas the context has to hold
};

// the dense replay: always, or where a launch has more frames than four per CU hold
inline bool flood_dense_launch(int dense, int m, int areas) { return dense > 0 || (dense < 0 && m > areas); }

// the exact replay of m frames on a lane
inline ExactLaunch exact_launch(const ChainPlan& p, int lane, int m)
{
	const int areas = p.lane[lane].areas;
	auto upto = [m](int instance, int cap) { const int grid = m < cap ? m : cap; return ExactLaunch{instance, grid, grid < m}; };
	// eight per CU: per-cell state as bits in LDS + bytes in global memory, a 4 160-slot LDS heap (CIMBAR_HIP_FLOOD_DENSE_GRID: fewer workgroups
	// than that, e.g. 1 792 = seven per CU, leave LDS for another stream's kernels while they run)
	if (flood_dense_launch(p.flood_dense, m, areas)) return upto(8, FLOOD_DENSE_PER * areas * p.flood_dense_grid / (FLOOD_DENSE_PER * FLOOD_GRID));
	// three frames per CU while the batch fits, four (smaller LDS heap) beyond that
	if (m <= areas * FLOOD_GRID3 / FLOOD_GRID) return ExactLaunch{3, m, false};
	return upto(4, areas);
}

inline ChainPlan plan_chain(const ChainPlanIn& in)
{
	ChainPlan p;
	const int n = in.n;
	// more than a quarter of the batch before took a flood kernel: two half-size exact replays on two queues run one after the other in effect
	const bool mostly_flood = in.flagged[1] != 0 && 4u * in.flagged[0] > in.flagged[1];
	const bool ordinary = !in.pipe && !in.timed && in.tail_split && n >= 64 * in.tail_parts;
	p.split = ordinary && !in.no_split && !mostly_flood;
	p.counted = ordinary && in.have_flagged;
	p.stop_at_mid = in.symbols_only && !in.pipe && !p.split;

	// The certifying pass costs ~2.5 us per flagged frame even when it gives up in its first super-round, which is what it does on every
	// deskewed camera frame (DESIGN.md, K2c). Where the batch before shows that it certified fewer than one in sixteen of the frames it was
	// given, the next fifteen batches go straight to the exact replay and the one after probes again. The decoded bytes do not depend on
	// this (both passes produce the reference's result); it only decides which kernel does the work.
	p.run_wave = in.flood_wave != 0;
	p.wave_ran = in.wave_ran;
	p.wave_skip_left = in.wave_skip_left;
	if (p.run_wave && p.counted && in.wave_adapt && !in.flood_verify) {
		const uint32_t f0 = in.flagged[0], replayed = in.flagged[2] <= f0 ? in.flagged[2] : f0;
		if (p.wave_skip_left > 0) { --p.wave_skip_left; p.run_wave = false; }
		else if (in.wave_ran && f0 >= 16u && 16u * (f0 - replayed) < f0) { p.run_wave = false; p.wave_skip_left = 14; }
	}
	if (p.counted) p.wave_ran = p.run_wave;
	// the relaxed flood takes the batch's own flags in threshold rounds; the verify replay exists only where the batch-parallel pass does
	p.exact_batch = !in.relaxed;
	p.exact_verify = in.flood_verify && in.flood_wave;
	p.exact_fallback = in.relaxed && in.relaxed_fallback;

	// The slots. The bases of the spill areas are spaced for the largest launch the context can make: FLOOD_DENSE_PER areas per ordinary one
	// wherever the dense replay may run at all (flood_dense != 0), whichever instance a launch takes -- a dense launch in one slot and an
	// ordinary one in another may be in flight together. The context holds every slot up to the last one that this kind of call may index,
	// sized by the whole batch (the parts of a split batch are smaller).
	const int ways = in.pipe ? in.pipe_depth : (p.split ? 2 : 1);
	const int areas = FLOOD_GRID / ways, wareas = FW_GRID / ways, scale = in.flood_dense != 0 ? FLOOD_DENSE_PER : 1;
	for (int l = 0; l < 2; ++l) {
		const int k = in.pipe ? in.pipe_set : (p.split ? l : 0);
		p.lane[l] = ChainLane{areas, scale * k * areas, wareas, k * wareas, k};
	}
	p.flood_dense = in.flood_dense;
	p.flood_dense_grid = in.flood_dense_grid;
	const int most = flood_dense_launch(in.flood_dense, n, areas) ? FLOOD_DENSE_PER * areas : areas;
	p.flood_top = scale * (ways - 1) * areas + (n < most ? n : most);

	// parts alternate between the two lanes; part q starts at frame n q / parts
	p.nparts = p.split ? in.tail_parts : 1;
	for (int q = 0; q < p.nparts; ++q) {
		const int lo = (int)((long long)n * q / p.nparts), hi = (int)((long long)n * (q + 1) / p.nparts);
		p.part[q] = ChainPart{lo, hi - lo, q & 1};
	}
	return p;
}

}  // namespace
