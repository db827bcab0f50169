// chain_plan_shim.cpp -- libcimbar_amd/csrc/chainplan.hip.inc behind a C symbol, for tests/test_chain_plan.py (g++, no HIP):
//     g++ -O2 -std=c++17 -shared -fPIC -o libchain_plan.so tools/chain_plan_shim.cpp
// chain_plan() plans one call and writes the exact-replay launches it stands for the way enqueue() issues them (host.hip.inc: every part in
// issue order, per part the replays exact_batch / exact_verify / exact_fallback), in CIMBAR_HIP_TAP_FLOOD_LAUNCH's record layout.
#include "../libcimbar_amd/csrc/chainplan.hip.inc"

extern "C" {

// in: {n, pipe, no_split, timed, flagged[0..2], tail_split, tail_parts, pipe_depth, pipe_set, dense, dense_grid, wave, verify, relaxed, fallback}
// recs: up to FLOOD_LAUNCH_MAX x {instance, grid, frames, first frame, area0, counter, flags}; lanes: the lane of each record
// head: {records, flood_top, split, counted, run_wave}; lane_out: 2 x {areas, area0, wareas, warea0, counter}
int chain_plan(const int32_t in_[17], int32_t recs[][7], int32_t* lanes, int32_t head[5], int32_t lane_out[2][5])
{
	ChainPlanIn in;
	in.n = in_[0]; in.pipe = in_[1]; in.no_split = in_[2]; in.timed = in_[3];
	in.have_flagged = true;
	for (int k = 0; k < 3; ++k) in.flagged[k] = (uint32_t)in_[4 + k];
	in.tail_split = in_[7]; in.tail_parts = in_[8]; in.pipe_depth = in_[9]; in.pipe_set = in_[10];
	in.flood_dense = in_[11]; in.flood_dense_grid = in_[12];
	in.flood_wave = in_[13]; in.flood_verify = in_[14];
	in.relaxed = in_[15]; in.relaxed_fallback = in_[16];
	const ChainPlan p = plan_chain(in);
	int count = 0;
	for (int q = 0; q < p.nparts; ++q) {
		const ChainPart& part = p.part[q];
		const bool kinds[3] = {p.exact_batch, p.exact_verify, p.exact_fallback};
		for (int kind = 0; kind < 3; ++kind) {
			if (!kinds[kind] || count >= FLOOD_LAUNCH_MAX) continue;
			const ExactLaunch x = exact_launch(p, part.lane, part.count);
			const int32_t rec[7] = {x.instance, x.grid, part.count, part.first, p.lane[part.lane].area0, p.lane[part.lane].counter, kind};
			for (int k = 0; k < 7; ++k) recs[count][k] = rec[k];
			lanes[count++] = part.lane;
		}
	}
	const int32_t h[5] = {count, p.flood_top, p.split, p.counted, p.run_wave};
	for (int k = 0; k < 5; ++k) head[k] = h[k];
	for (int l = 0; l < 2; ++l) {
		const ChainLane& L = p.lane[l];
		const int32_t v[5] = {L.areas, L.area0, L.wareas, L.warea0, L.counter};
		for (int k = 0; k < 5; ++k) lane_out[l][k] = v[k];
	}
	return count;
}

int chain_plan_constants(int32_t out[6])
{
	const int32_t v[6] = {FLOOD_GRID, FLOOD_GRID3, FLOOD_DENSE_PER, FW_GRID, FLOOD_COUNTERS, FLOOD_LAUNCH_MAX};
	for (int k = 0; k < 6; ++k) out[k] = v[k];
	return 6;
}

}
