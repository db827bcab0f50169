// mode.hip.inc -- everything that depends on the frame geometry: constants, kernels, context and host logic. Included by cimbar_hip.hip once per
// supported mode with CIMBAR_MODE / CIMBAR_NS set; each copy lives in its own namespace (m68, m67, m66, m4, m8) and api.hip.inc dispatches the C ABI on the
// context's mode.
namespace CIMBAR_NS __attribute__((visibility("hidden"))) {

namespace {

// ------------------------------------------------------------------------------------------------ grid constants
// The geometry is a compile-time parameter set (the kernels' strip layout, LDS sizes and unrolling depend on it): this file is compiled once
// per supported mode, 68 = "B" (Conf8x8, lib/cimb_translator/GridConf.h:121-142), 67 = "Bm" (Conf8x8_mini, GridConf.h:168-189) and 66 = "Bu"
// (Conf8x8_micro, GridConf.h:144-166). Everything else follows Config.h:101-165. CHUNKS = fountain_chunks_per_frame = 6 bits per cell *
// fountain_chunks_scalar (GridConf.h:54-61); K1_CELLROWS / K1_TALLROWS = cell rows per threshold strip of the two K1 instances (k1_threshold.hip.inc: short strips for a launch that
// runs alone, tall ones inside the pipelined loop).
#ifndef CIMBAR_K1_TALLROWS_BM
#define CIMBAR_K1_TALLROWS_BM 5      // (mode 67, 78 cell rows: 16 strips, the last one of three rows; measured on one box, three rounds: short strips 0.507-0.522 ms per step, 3: 0.497-0.514, 5: 0.488-0.499, 6: 0.524-0.533; 13 on another box: 0.597 against 0.553 for 6)
#endif
#ifndef CIMBAR_K1_PPL_BU
#define CIMBAR_K1_PPL_BU 12         // (mode 66: pixels per lane of the threshold pass, 16 | 12 -- k1_threshold.hip.inc; 736-pixel rows fill 46 lanes at 16, 61 1/3 at 12)
#endif
#ifndef CIMBAR_K1_TALLROWS_B
#define CIMBAR_K1_TALLROWS_B 7      // (A/B builds: -DCIMBAR_K1_TALLROWS_B=6 | 8 | 10, see k1_threshold.hip.inc)
#endif
#if CIMBAR_MODE == 68
constexpr int IMG_W = 1024, IMG_H = 1024, OFFSET = 8, DIM_X = 112, DIM_Y = 112, RS_BLOCK = 155, RS_PARITY = 30, CHUNKS = 12, K1_CELLROWS = 2, K1_TALLROWS = CIMBAR_K1_TALLROWS_B;
#elif CIMBAR_MODE == 67
constexpr int IMG_W = 1024, IMG_H = 720, OFFSET = 9, DIM_X = 112, DIM_Y = 78, RS_BLOCK = 179, RS_PARITY = 36, CHUNKS = 12, K1_CELLROWS = 2, K1_TALLROWS = CIMBAR_K1_TALLROWS_BM;
#elif CIMBAR_MODE == 66
constexpr int IMG_W = 736, IMG_H = 637, OFFSET = 9, DIM_X = 80, DIM_Y = 69, RS_BLOCK = 168, RS_PARITY = 33, CHUNKS = 6, K1_CELLROWS = 3, K1_TALLROWS = 6;   // (measured short / tall 2 / 4, 3 / 4, 4 / 8, 5 / 12: 0.386, 0.386, 0.382, 0.424 ms per step against 0.373-0.376)
#elif CIMBAR_MODE == 4   // Config.h:24-29: Conf8x8 with legacy_mode -- coupled decode (Decoder.h:121-161), colour_mode 0 palette, ten chunks per frame
constexpr int IMG_W = 1024, IMG_H = 1024, OFFSET = 8, DIM_X = 112, DIM_Y = 112, RS_BLOCK = 155, RS_PARITY = 30, CHUNKS = 10, K1_CELLROWS = 2, K1_TALLROWS = 7;
#elif CIMBAR_MODE == 8   // Config.h:30-35: the same with 3 colour bits (7-bit cells, 70 blocks, the eight colours of getColor8_old)
constexpr int IMG_W = 1024, IMG_H = 1024, OFFSET = 8, DIM_X = 112, DIM_Y = 112, RS_BLOCK = 155, RS_PARITY = 30, CHUNKS = 10, K1_CELLROWS = 2, K1_TALLROWS = 7;
#else
#error "CIMBAR_MODE must be 68 (Conf8x8), 67 (Conf8x8_mini), 66 (Conf8x8_micro), 4 or 8 (legacy 4- / 8-colour)"
#endif
constexpr int MODE_VAL = CIMBAR_MODE;
// legacy_mode: a cell's 2 colour + 4 symbol bits travel as ONE 6-bit field of ONE Reed-Solomon stream (no separate colour stream, hence no
// fountain header before the colour pass and no header-derived colour correction)
constexpr bool LEGACY = CIMBAR_MODE == 4 || CIMBAR_MODE == 8;
constexpr int COLOR_BITS = CIMBAR_MODE == 8 ? 3 : 2, NCOLORS = 1 << COLOR_BITS, CELL_BITS = 4 + COLOR_BITS;
// the row passes map lane l of a wavefront onto pixels [PPL l, PPL l + PPL): rows of up to 1024 pixels, a multiple of 16 wide; lanes beyond
// LAST_LANE idle (they load what LAST_LANE loads and their results are never read). The frame renderer holds 16 pixels per lane (ROW16_LAST_LANE),
// the threshold pass K1_PPL: 16, or 12 where that fills more of the wavefront (mode 66); LAST_PX = the pixels of the row in its last lane
static_assert(IMG_W % 16 == 0 && IMG_W <= 1024, "the row passes map 64 lanes x 16 pixels onto a row");
constexpr int K1_PPL = CIMBAR_MODE == 66 ? CIMBAR_K1_PPL_BU : 16;
constexpr int ROW16_LAST_LANE = IMG_W / 16 - 1;
constexpr int LAST_LANE = (IMG_W + K1_PPL - 1) / K1_PPL - 1, LAST_PX = IMG_W - LAST_LANE * K1_PPL;
static_assert(LAST_LANE <= 63, "one wavefront per row");
constexpr int PLANE_ROW = 32;                                            // u32 words per bit-plane row, whatever the width (bits >= IMG_W are never read)
constexpr int PITCH = 9, MARKER = 6;                                     // cell_spacing, corner_padding = lrint(54 / 9) (GridConf.h:17-40)
constexpr int TOP_W = DIM_X - 2 * MARKER;                                // 100
constexpr int TOP_CELLS = TOP_W * MARKER;                                // 600
constexpr int MID_CELLS = DIM_X * (DIM_Y - 2 * MARKER);                  // 11200 | 7392
constexpr int NCELLS = DIM_X * DIM_Y - 4 * MARKER * MARKER;              // 12400 | 8592 (GridConf.h:42-45)
constexpr int RS_DATA = RS_BLOCK - RS_PARITY;                            // 125 | 143
constexpr int SYM_BLOCKS = LEGACY ? NCELLS * CELL_BITS / 8 / RS_BLOCK : NCELLS * 4 / 8 / RS_BLOCK;   // legacy: the one coupled stream's blocks count as "symbol" blocks
constexpr int COL_BLOCKS = LEGACY ? 0 : NCELLS * 2 / 8 / RS_BLOCK, ALL_BLOCKS = SYM_BLOCKS + COL_BLOCKS;   // 40 + 20 | 24 + 12 | 16 + 8 | 60 + 0
constexpr int CHUNK = ALL_BLOCKS * RS_DATA / CHUNKS, FRAME_BYTES = CHUNK * CHUNKS;   // 625 | 429 | 540 (GridConf.h:63-71)
constexpr int BLOCKS_PER_CHUNK = CHUNK / RS_DATA;                        // 5 | 3 | 4
constexpr int SYM_CHUNKS = SYM_BLOCKS / BLOCKS_PER_CHUNK, COL_CHUNKS = COL_BLOCKS / BLOCKS_PER_CHUNK;   // 8 + 4 | 8 + 4 | 4 + 2
constexpr int NHDR = CHUNKS / 3, NHDR_CELLS = NHDR * 24;                 // fountain headers the colour stream carries at known cells (CimbReader.cpp:188-227): 4 | 4 | 2
static_assert((LEGACY ? NCELLS * CELL_BITS / 8 % RS_BLOCK == 0 : (NCELLS * 4 / 8 % RS_BLOCK == 0 && NCELLS * 2 / 8 % RS_BLOCK == 0)) && CHUNK % RS_DATA == 0 &&
              ALL_BLOCKS * RS_DATA == FRAME_BYTES, "mode arithmetic");
static_assert(SYM_CHUNKS * BLOCKS_PER_CHUNK == SYM_BLOCKS && COL_CHUNKS * BLOCKS_PER_CHUNK == COL_BLOCKS && SYM_CHUNKS + COL_CHUNKS == CHUNKS && (LEGACY || SYM_BLOCKS <= 64) &&
              SYM_CHUNKS * 6 <= 64, "chunks end on block boundaries; block flags and the symbol chunks' header bytes fit one wavefront");
constexpr int PLANE_WORDS = PLANE_ROW * IMG_H;                           // u32 per frame
constexpr size_t FRAME_RGB = (size_t)IMG_W * IMG_H * 3;
constexpr int ANCHOR = 30;
constexpr int HEAP_CAP = 12 * NCELLS + 64;            // <= 12 offers per decoded cell + 8 seeds

// the 16 tile hashes and the exact-match slot table of k_symbols: computed by cimbar_hip_create from the tile bitmaps the way
// CimbDecoder's constructor does (CimbDecoder.cpp:58-66,87-99 -> Common.cpp:150-171 getTile -> average_hash.h:19-39), see
// build_tile_hashes() in host.hip.inc
__constant__ uint64_t c_tile[16];

// Common.cpp:21-31 getColor4 (colour_mode 1); legacy modes: colour_mode 0 = getColor4_old (Common.cpp:45-54)
#if CIMBAR_MODE == 8   // getColor8_old (Common.cpp:71-84)
__constant__ int c_palette[8][3] = {{0, 255, 255}, {127, 127, 255}, {255, 0, 255}, {255, 65, 65}, {255, 159, 0}, {255, 255, 0}, {255, 255, 255}, {0, 255, 0}};
#elif CIMBAR_MODE == 4
__constant__ int c_palette[4][3] = {{0, 255, 255}, {255, 255, 0}, {255, 0, 255}, {0, 255, 0}};
#else
__constant__ int c_palette[4][3] = {{0, 255, 0}, {0, 255, 255}, {255, 255, 0}, {255, 0, 255}};
#endif

// GF(2^8), primitive poly 0x187 (libcorrect field.h:26-62): exp[512], log[256]
__constant__ uint8_t c_gf_exp[512];
__constant__ uint8_t c_gf_log[256];

struct Tables {
	ushort2* cell_xy;        // [NCELLS] top-left pixel of each cell (CellPositions.cpp:5-51)
	uint16_t* stream_cell;   // [NCELLS] stream index -> linear cell index (Interleave.h:8-24)
	uint16_t* cell_grid;     // [NCELLS] grid slot (row * 112 + col) of each cell: where K1 left its 6x6 colour mean
	int16_t* grid_cell;      // [DIM_X * DIM_Y] the inverse: linear cell index of a grid slot, -1 inside the four corner cut-outs (k_colors walks the slots)
	uint16_t* ccm_grid;      // [NHDR_CELLS = 96 | 48] grid slot (row * 112 + col) of the cells whose colour the fountain header predicts: colour-stream
	                         // cells 3100*c + t, t < 24 (CimbReader.cpp:188-227)
	int16_t* cand;           // [NCELLS][12] the cells FloodDecodePositions::update may offer to, in its order: right, left, bottom,
	                         // top (AdjacentCellFinder.cpp:16-105), then the 4 horizontal and 4 vertical "horizon" cells
	                         // (FloodDecodePositions.cpp:93-129); -1 = none
};

#include "k1_threshold.hip.inc"
#include "k2_symbols.hip.inc"
#include "k2b_flood.hip.inc"
#include "k2c_floodwave.hip.inc"
#include "k2d_floodrounds.hip.inc"
#include "k3_rs.hip.inc"
#include "k4_frame.hip.inc"
#include "erasure.hip.inc"
#include "combine.hip.inc"
#include "stitch.hip.inc"
#include "repeat.hip.inc"
#include "k1_padded.hip.inc"
#include "encode.hip.inc"
#include "extract.hip.inc"
#include "scan.hip.inc"
#include "undistort.hip.inc"

}  // namespace

#include "host.hip.inc"
#include "automode_mode.hip.inc"

}  // namespace CIMBAR_NS
