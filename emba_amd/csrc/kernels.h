// emba_amd/csrc/kernels.h — hand-written HIP kernels (gfx950 / CDNA4, wave64) for the EMBA hot path.
//
// Data layout in HBM:
//   events    pixel-major (sensor pixel, then time): ev_pix u32 (bit31 = polarity), ev_batch u32,
//             ev_slot u32 (factor-record slot, kNoSlot if the event has no predecessor at its pixel)
//   pose      one 112-B record per 100-event batch: q[4] J1[9] cp   (R = matrix(q) per event like rot.matrix() at
//             event_pano_warper.cpp:55; J0 = I - J1)
//   texel     per panorama pixel {Gx Gy Gxx Gxy Gyy pad} = 48 B   (one gather per measurement)
//   records   one 128-B factor record per measurement candidate, stored in (cp_c,cp_p)-sorted slots:
//             jc[6] jp[6] dp[2] e {u32 pano_idx, u32 evaluation stamp}  — the sparse A12 factor + what A11/A22 need; only inliers
//             are written, a slot is valid iff its stamp is the current evaluation's (record_valid)
//   pixacc    per panorama pixel 64 B {sum w dx*dx, w dx*dy, w dy*dy, dx*we, dy*we, n, pad x2}: the A22/b2 sums (IRLS-weighted when
//             the cost is declared) and the COUNT of every inlier measurement — one atomic request per measurement; the int32
//             count map only gets a marker from the warp kernel and is materialised from these lines by the next dense pass;
//             only touched lines are ever non-zero and they are cleared again by emba_prep_kernel at the start of the next evaluation
//   pack      [A11 (3K)^2 col-major | b1 3K | per active pixel {xx xy yy bx by}]  (one all-reduce)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.h"
#include "order_rule.h"   // ChunkDesc, TileShape
#include "step_rule.h"    // kRectMargin, rect_contained

// Development ablations (EMBA_ABLATE bit mask: parts of a kernel switched off to see what they cost; results are WRONG when non-zero)
// exist only in a diagnostics build (-DEMBA_DIAG, scripts/ablate*.sh build one under build_variants/): the shipped library has none of
// the branches and does not read the variable.
#ifdef EMBA_DIAG
#define EMBA_ABL(word, bit) (((word) & (bit)) != 0)
#else
#define EMBA_ABL(word, bit) false
#endif

namespace emba {

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kInvalidPix = 0xFFFFFFFFu;

// A factor record is valid for the CURRENT evaluation iff its tail word carries this evaluation's stamp: the warp kernel only
// writes the records of inliers (full 128-B lines), an outlier's slot keeps whatever an earlier evaluation left there.
__device__ __forceinline__ bool record_valid(double tail_y, uint32_t stamp, uint32_t& pano_idx)
{
    pano_idx = (uint32_t)__double2loint(tail_y);
    return (uint32_t)__double2hiint(tail_y) == stamp && pano_idx != kInvalidPix;
}
// The count-map entry of a pixel the evaluation with this stamp touched, until the next dense pass replaces it by the pixel's count
// (materialise_mask8): negative, so it is never a count, and stamped, so that whatever an EARLIER evaluation left in the map — its
// counts, or markers nobody materialised — reads as "not touched" without the map having been cleared in between.
__host__ __device__ __forceinline__ int32_t count_marker(uint32_t stamp) { return (int32_t)(0x80000000u | (stamp & 0x3FFFFFFFu)); }
constexpr int kPoseStride = 14;    // doubles per pose record: q[4] J1[9] cp  (112 B = 7 x 16-B gathers per event)
#ifndef TEXEL_STRIDE
#define TEXEL_STRIDE 6
#endif
constexpr int kTexelStride = TEXEL_STRIDE;    // doubles per texel
constexpr int kRecStride = 16;     // doubles per factor record
constexpr int kWarpBlock = 64;     // the warp kernel's workgroup is ONE wave: no barriers, neighbours talk through DPP
constexpr int kWarpNew = 63;       // new events per wave (lane 0 re-warps the predecessor of lane 1)
constexpr int kRecLds = 18;        // doubles per record in the LDS staging tile (144 B: conflict-free 16-B accesses)
constexpr int kPixAccStride = 8;  // doubles per pixacc line (64 B)
// Streaming accesses marked non-temporal (they are written / read once per launch and should not displace the gather tables —
// bearing vectors, texels, segment records, activity bits — from L2): REC_NT_STORE the 128-B record stores of the warp kernels
// (measured: 10 M events 514 -> 467 us, 100 M 4.70 -> 4.46 ms, and the Gram kernel after it 309 -> 283 us), EP_NT_STORE the
// residual / flag stores, GRAM_NT_LOAD the Gram kernel's record stream, EV_NT_LOAD the event-word stream.
#ifndef REC_NT_STORE
#define REC_NT_STORE 1
#endif
#ifndef EP_NT_STORE
#define EP_NT_STORE 1     // 10 M: 496 -> 481 us, 100 M: 4.54 -> 4.40 ms, 1 M: equal
#endif
#ifndef GRAM_NT_LOAD
#define GRAM_NT_LOAD 1    // Gram kernel, 10 M: 293 -> 269 us, 100 M: 2.65 -> 2.58 ms
#endif
#ifndef EV_NT_LOAD
#define EV_NT_LOAD 1      // TILE ORDER ONLY (10 M: 496 -> 484 us); in pixel order at 1 M events the words are Infinity-Cache hits and NT loads cost 52 -> 72 us
#endif
#ifndef GRAM_TAG_NT
#define GRAM_TAG_NT 0
#endif
template <class T> __device__ __forceinline__ T stream_load(const T* p, bool nt) { return nt ? __builtin_nontemporal_load(p) : *p; }
#ifndef GRAM_DUMMY_LOADS
#define GRAM_DUMMY_LOADS 0   // 1: dead records are loaded from one fixed line instead of skipped (exact wait counts; measured 4 % slower at 10 M events, equal at 1 M)
#endif
#ifndef GRAM_U_NT
#define GRAM_U_NT 3
#endif
#ifndef GRAM_U
#define GRAM_U 4
#endif
#ifndef GRAM_SPARSE_TS
#define GRAM_SPARSE_TS 2         // sparse form: tag loads (64 slots each) per wave and stage.  10 M events on 2048 x 4096: 1: 97-102 us, 2: 77-79, 3: 79-81, 4: 93-110 (64 B of scratch), 8: 170
#endif
constexpr int kGramPad = 256;     // record slots allocated past the last one: the Gram kernel's stages read whole 8-record groups
constexpr int kGramChunkMin = 64; // smallest share of record slots a wave of the Gram kernel is given
constexpr int kGramChunk = 1024;   // most record slots a wave of the Gram (A11/b1) kernel is given (multiple of 8)
#ifndef GATHER_Q
#define GATHER_Q 4
#endif
#ifndef GRAM_GATHER_WAVES
#ifndef GRAM_WAVE_TILE
#define GRAM_WAVE_TILE 1         // a wave's last flush goes to its own LDS tile by plain stores (gram_wave_tile) instead of fp64 LDS atomics into the block's table
#endif
#define GRAM_GATHER_WAVES 4      // waves of a Gram block that do its slice of the active-set gather while the other 12 stream records (GATHER form)
#endif
constexpr int kGramBlock = 1024;   // threads per block of the Gram kernel (16 waves share one LDS combine table).  Round 4, compact form at 1 M events: 8 waves
                                   // per CU 52 us, 4 waves 93 us, 24 waves (768 x 2, 80 VGPRs, 13 spilled) 39.6 us, 32 waves (64 VGPRs, 81 spilled) 52-66 us; 16: 37 us
constexpr int kGramKeys = 4;       // control-pose pairs the block-level LDS table can hold before falling back to global atomics

// Blocks are dealt round-robin over the 8 XCDs (MI355X_MICROARCH.md "Workgroup dispatch"); give each
// XCD a contiguous range of work so that neighbouring sensor pixels (= neighbouring panorama texels,
// count-map and A22 lines) share one L2.  Speed only, never correctness.
__device__ __forceinline__ long xcd_contiguous_block(long bid, long grid)
{
    const long per = grid >> 3;  // grid is a multiple of 8
    return (bid & 7) * per + (bid >> 3);
}

// ------------------------------------------------------------------------------------------------
// a2/a3: one thread per batch -> pose record.  LinearTrajectory::evaluate (trajectory.cpp:122-147) /
// So3Spline<2>::evaluate (so3_spline.h:218-274).  s and u use the same int64 arithmetic as the reference.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pose_thread(int b, const int64_t* __restrict__ batch_t_ns, int nb, const double* __restrict__ knots,
                                            int K, int64_t t0_ns, int64_t dt_ns, double* __restrict__ pose, int* __restrict__ err)
{
    if (b >= nb) return;
    const int64_t st = batch_t_ns[b] - t0_ns;
    const int64_t s = (st >= 0) ? st / dt_ns : -1;
    if (st < 0 || s + 2 > (int64_t)K) {  // BASALT_ASSERT_STREAM at so3_spline.h:221-229
        atomicOr(err, 1);
        return;
    }
    const double u = (double)(st % dt_ns) / (double)dt_ns;
    double p0[4], p1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { p0[i] = knots[4 * s + i]; p1[i] = knots[4 * (s + 1) + i]; }
    double q[4], J1[9];
    spline2_eval(p0, p1, u, q, J1);
    double* o = pose + (size_t)kPoseStride * b;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = q[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) o[4 + i] = J1[i];
    o[13] = (double)s;
}

// Tile order: per-SEGMENT constants instead (device_math.h: segment_consts / spline2_event); thread s fills segment s of seg[12 s].
constexpr int kSegStride = kSegRecordDoubles;   // (seg_record_rule.h: the host strides its records by the same constant)
static_assert(kSegStride == 12, "a record is {p0[4], delta[3], r1, k[3], r2}");
// (the record of segment sidx as VALUES: whoever forms it — the prep launch, workgroup 0 of the warp launch, a wave that gave up waiting for that one — gets the
// same bits, and nothing downstream is contracted into the chain: the values pass through registers the compiler cannot see into)
__device__ __forceinline__ void seg_record(int sidx, const double* __restrict__ knots, double* __restrict__ o)
{
    double p0[4], p1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { p0[i] = knots[4 * sidx + i]; p1[i] = knots[4 * (sidx + 1) + i]; }
    segment_consts(p0, p1, o);
#pragma unroll
    for (int i = 0; i < kSegStride; ++i) __asm__ volatile("" : "+v"(o[i]));
}
__device__ __forceinline__ void seg_thread(int sidx, const double* __restrict__ knots, int K, double* __restrict__ seg)
{
    if (sidx >= K - 1) return;
    double o[kSegStride];
    seg_record(sidx, knots, o);
#pragma unroll
    for (int i = 0; i < kSegStride; ++i) seg[(size_t)kSegStride * sidx + i] = o[i];
}

__global__ __launch_bounds__(64) void emba_pose_kernel(const int64_t* __restrict__ batch_t_ns, int nb, const double* __restrict__ knots, int K,
                                                       int64_t t0_ns, int64_t dt_ns, double* __restrict__ pose, int* __restrict__ err)
{
    pose_thread(blockIdx.x * 64 + threadIdx.x, batch_t_ns, nb, knots, K, t0_ns, dt_ns, pose, err);
}

// ------------------------------------------------------------------------------------------------
// a1: texel pack.  0.125*Sobel3x3 with BORDER_REFLECT_101, Gxy := (dGx/dy + dGy/dx)/2 (model.cpp:88-97),
// fused with the AoS interleave so that one measurement gathers one 48-B texel instead of 5 planes.
// HBM-bound: reads 16 B/pixel (neighbours from L1/L2), writes 48 B/pixel.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect101(int i, int n)
{
    if (n == 1) return 0;
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

// Hessian stencil at (x,y); the arithmetic (and its order) is shared by the texel pack and by the on-the-fly path.
__device__ __forceinline__ void hessian_at(const double* __restrict__ Gx, const double* __restrict__ Gy, int H, int W, int x, int y,
                                           double& g_x, double& g_y, double& gxx_o, double& gxy_o, double& gyy_o)
{
    const int xl = reflect101(x - 1, W), xr = reflect101(x + 1, W);
    const int yu = reflect101(y - 1, H), yd = reflect101(y + 1, H);
    const double* gxu = Gx + (size_t)yu * W; const double* gxc = Gx + (size_t)y * W; const double* gxd = Gx + (size_t)yd * W;
    const double* gyu = Gy + (size_t)yu * W; const double* gyc = Gy + (size_t)y * W; const double* gyd = Gy + (size_t)yd * W;
    // d/dx: rows [-1 0 1], columns [1 2 1]
    const double gxx = ((gxu[xr] - gxu[xl]) + (gxd[xr] - gxd[xl])) + 2 * (gxc[xr] - gxc[xl]);
    const double gyx = ((gyu[xr] - gyu[xl]) + (gyd[xr] - gyd[xl])) + 2 * (gyc[xr] - gyc[xl]);
    // d/dy: rows [1 2 1], columns [-1 0 1]
    const double gxy = ((gxd[xl] + gxd[xr]) + 2 * gxd[x]) - ((gxu[xl] + gxu[xr]) + 2 * gxu[x]);
    const double gyy = ((gyd[xl] + gyd[xr]) + 2 * gyd[x]) - ((gyu[xl] + gyu[xr]) + 2 * gyu[x]);
    g_x = gxc[x]; g_y = gyc[x];
    gxx_o = 0.125 * gxx;
    gxy_o = 0.5 * (0.125 * gxy + 0.125 * gyx);
    gyy_o = 0.125 * gyy;
}

// Texel rectangle: the bounding box (+ kRectMargin, step_rule.h) of the pixels an EARLIER formed evaluation touched, reduced by its active-set write.
// Inside it the warp kernel gathers one 48-B texel (3 cache accesses); outside it falls back to the 3x3 stencil on the Gx/Gy
// planes (18 accesses).  Consecutive LM trial points move the footprint by a few pixels, so almost every gather is a texel.
// rect = {x0, y0, x1, y1} inclusive; empty if x1 < x0.  acc = raw {xmin, ymin, xmax, ymax}: the box the texels were last PACKED for (the pack's
// block 0 copies it from the newest box; texels are packed when they are stale, not in every evaluation: step_rule.h, texels_stale).
__device__ __forceinline__ void texel_rect(const int* __restrict__ acc, int W, int H, int& x0, int& y0, int& x1, int& y1)
{
    const int ax0 = acc[0], ay0 = acc[1], ax1 = acc[2], ay1 = acc[3];
    if (ax1 < ax0 || ay1 < ay0) { x0 = 0; y0 = 0; x1 = -1; y1 = -1; return; }
    x0 = max(ax0 - kRectMargin, 0); y0 = max(ay0 - kRectMargin, 0);
    x1 = min(ax1 + kRectMargin, W - 1); y1 = min(ay1 + kRectMargin, H - 1);
}

__device__ __forceinline__ void texel_rect_blocks(long blk, long nblocks, const double* __restrict__ Gx, const double* __restrict__ Gy,
                                                  int H, int W, const int* __restrict__ rect_acc, double* __restrict__ texel)
{
    // rect_acc: the box of the pixels the last formed evaluation touched (reduced by its active-write kernel's last block)
    int x0, y0, x1, y1;
    texel_rect(rect_acc, W, H, x0, y0, x1, y1);
    const long rw = x1 - x0 + 1, total = rw * (long)(y1 - y0 + 1);
    for (long idx = blk * 256 + threadIdx.x; idx < total; idx += nblocks * 256) {
        const int x = x0 + (int)(idx % rw), y = y0 + (int)(idx / rw);
        double gx, gy, gxx, gxy, gyy;
        hessian_at(Gx, Gy, H, W, x, y, gx, gy, gxx, gxy, gyy);
        double2* t = reinterpret_cast<double2*>(texel + (size_t)kTexelStride * ((size_t)y * W + x));
        t[0] = make_double2(gx, gy);
        t[1] = make_double2(gxx, gxy);
        t[2] = make_double2(gyy, 0.0);
    }
}

__global__ __launch_bounds__(256) void emba_texel_kernel(const double* __restrict__ Gx, const double* __restrict__ Gy,
                                                         int H, int W, double* __restrict__ texel)
{
    // One texel per thread; the 48-B texels of a wave go through LDS so that the wave writes its 3 KB as three fully coalesced 1-KB
    // stores (16 B per lane, consecutive lanes) instead of three stores that each touch every line of the span partially.
    static_assert(kTexelStride == 6, "three 16-B pieces per texel");
    __shared__ __attribute__((aligned(16))) double s_t[4][64 * kTexelStride];
    const int x0 = blockIdx.x * blockDim.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = x0 + threadIdx.x;
    const int y = blockIdx.y;
    double gx = 0, gy = 0, gxx = 0, gxy = 0, gyy = 0;
    if (x < W) hessian_at(Gx, Gy, H, W, x, y, gx, gy, gxx, gxy, gyy);
    double2* l = reinterpret_cast<double2*>(s_t[wv] + kTexelStride * lane);
    l[0] = make_double2(gx, gy); l[1] = make_double2(gxx, gxy); l[2] = make_double2(gyy, 0.0);
    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // (one wave reads what it wrote itself: LDS operations complete in order)
    const int xw = x0 + 64 * wv;                                // first texel of this wave
    const int n_tex = (W - xw < 64) ? (W - xw) : 64;           // texels of this wave inside the row
    if (n_tex <= 0) return;
    double2* out = reinterpret_cast<double2*>(texel + (size_t)kTexelStride * ((size_t)y * W + xw));
    const double2* in = reinterpret_cast<const double2*>(s_t[wv]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = 64 * k + lane;                            // 16-B piece i of the wave's 3 * 64 pieces
        if (i < 3 * n_tex) out[i] = in[i];
    }
}

// ------------------------------------------------------------------------------------------------
// a4-a7 (+ the per-measurement half of a9): the dominant kernel, in two forms that share every per-event expression.
// One lane per entry of the device-order event array: gather the batch pose, warp (event_pano_warper.cpp:43-74 +
// equirectangular_camera.h:18-45), chain the Jacobian (model.cpp:155-157), hand pm to the next lane (the predecessor at the
// same sensor pixel is the previous array element whenever the entry's kEvHasPred bit says so), then pairing / outlier test /
// rounding / texel gather / residual / count (model.cpp:186-242) and the two 1x6 rows j_c = temp*D_k, j_p = -Gpm*D_{k-1}
// (model.cpp:449,459) written as one 128-B record.
//   emba_warp_residual_kernel  pixel order: one-wave workgroups, per-pixel sums straight to HBM (one atomic request per run)
//   emba_warp_tiled_kernel     tile order (order_kernels.h): a workgroup owns one panorama tile's worth of events and keeps the
//                              per-pixel sums of the tile (+ margin) in LDS; one atomic request per touched pixel at the end
// ------------------------------------------------------------------------------------------------
// LDS accumulator tile of the tiled kernel: 1152 panorama pixels x 6 doubles = 54 KB, two workgroups per CU.  Round 6: four shapes of that budget, one kernel
// instantiation each; a window takes the shape that cuts its chains into the fewest segments (order_kernels.h: the window rule; order_host.h: prepare_order).
// {tile w, h, pitch of the tile-origin grid, its finer variant for very dense windows}
constexpr int kNumTileShapes = 4;
constexpr TileShape kTileShapes[kNumTileShapes] = {
    {48, 24, 32, 8, 16, 4},      // the shape of rounds 2-5 (then: a 32 x 8 bin + 8 px of margin)
    {72, 16, 48, 4, 24, 4},      // fast pans
    {96, 12, 64, 4, 32, 2},
    {36, 32, 24, 8, 12, 8},      // trajectories that pitch
};
#ifndef TILE_WAVES
#define TILE_WAVES 8
#endif
#ifndef TILE_OCC
#define TILE_OCC 4
#endif
constexpr int kTileWaves = TILE_WAVES;          // waves per workgroup of the tiled kernel; two workgroups per CU (2 x 74 KB of LDS) = TILE_OCC waves per SIMD
constexpr int kTileRecStage = 16;               // records staged per wave at a time in the tiled kernel (a quarter of a wave)

struct WarpParams {
    const uint32_t* ev_pix; const uint32_t* ev_batch; const uint32_t* ev_slot; const uint32_t* ev_pm; long n_sorted; long nblk;   // ev_pm: entry -> pm-order index (nullptr: identity)
    const double* ev_u; const uint16_t* ev_seg;   // per entry the spline parameter u and the segment of its batch (the pose is evaluated per event from them)
    const double* pose; const double* seg; const double* lut; const double* texel;  // texel == nullptr: Hessian on the fly from Gx, Gy; pose: per-batch table (pixel order); seg: per-segment records (tile order)
    const int* rect_acc;   // non-null: texels are valid only inside texel_rect(rect_acc); stencil fallback outside
    const double* Gx; const double* Gy;
    int W, H; double fx, fy, cx, cy, C_th, outlier_px;
    int32_t* count; double* pixacc; double* rec; double* tag; double* e_sorted; uint8_t* flag;   // tag: 8 B per record slot {pano pixel, stamp}, or nullptr
    int* err;   // the step's status word: bit 0 = a batch outside the knots; bits 1.. = inliers the tiled kernel found OUTSIDE their tile (drift of the trajectory since the order was built)
    double* d_pm; double* d_D; double* d_dp; double* d_Gpm; double* d_temp; int32_t* d_pm_int;  // DUMP only
    int rec_nt;  // record stores non-temporal (windows whose records do not fit the Infinity Cache)
    int ablate;  // diagnostics only (EMBA_ABLATE): 1 no count marker, 2 no record store, 4 no texel gather, 8 no pixacc atomics
    int irls; double eta;   // robust cost the per-pixel sums are weighted with (0 quadratic: w = 1), model.cpp:599-636
    uint32_t stamp;         // evaluation number written into every record's tail word (see record_valid)
    int32_t marker;         // what a touched pixel's count-map entry is set to: count_marker(stamp), negative — never a count, never another evaluation's marker
    const ChunkDesc* chunks; long n_chunks; int chunks_linear;   // tiled kernel only; chunks_linear: chunk = blockIdx (the list is in dispatch order: longest first)
};

// lane l <- lane l-1 (lane 0 <- 0): one v_mov_b32_dpp wave_shr:1 per dword, no LDS
__device__ __forceinline__ int dpp_shr1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ double dpp_shr1(double v)
{
    return __hiloint2double(dpp_shr1(__double2hiint(v)), dpp_shr1(__double2loint(v)));
}
// lane l <- lane l+1 (lane 63 <- 0): wave_shl:1
__device__ __forceinline__ int dpp_shl1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, false); }
__device__ __forceinline__ double dpp_shl1(double v)
{
    return __hiloint2double(dpp_shl1(__double2hiint(v)), dpp_shl1(__double2loint(v)));
}

// The control poses of a spline with K <= kInlineKnots travel BY VALUE in the kernel arguments (emba_prep_pose_texel_kernel, emba_warp_residual_inline_kernel)
constexpr int kInlineKnots = 104;
struct InlineKnots { double q[4 * kInlineKnots]; };

// ---- the segment records INSIDE the pixel-order warp launch (step_rule.h: prep_inside_warp) -----------------------------------------------------------------
// What is left of the launch in front of the warp kernel on clean lines and fresh texels is one block that writes K - 1 records of 96 B.  Here workgroup 0 — the
// first dispatched — forms them from the control poses in the kernel arguments (seg_record: the prep launch's own chain, the same bits) and hands them to every
// other workgroup of the launch; it also takes over block 0's other duties (the next evaluation's status word, the device copy of the control poses).
// The hand-off (MI355X: eight XCDs with private L2s, an L1 per CU that no other CU's store refreshes):
//   producer   the records go out as write-through 8-B agent-scope stores, the wave drains them (vmcnt(0)), then ONE lane stores the flag — the number of this
//              hand-off on the context (it skips 0, the word's first value), which no earlier evaluation has written, so nothing is cleared between
//              evaluations — as an agent-scope store.  The number and the control poses are kernel ARGUMENTS: a captured graph would replay both frozen, and
//              the step is not captured (its poses change with every call).  Every shared word is reached through a global (address space 1) pointer
//   consumers  issue the loads that do not depend on the records (event words, spline parameter, segment, slot), then poll the flag with agent-scope loads and read
//              the records with 16-B sc1 buffer loads, EVERY load of them: a line an earlier evaluation left in this CU's L1 is never looked at.  No acquire: an
//              acquire per one-wave workgroup would be 15.9 k invalidations per launch at 1 M events
//   bounded    after `polls` polls a wave turns producer itself: it forms all K - 1 records (seg_record again: the same bits) and stores them the same way — the same
//              values to the same addresses, whoever else is writing them —, drains, counts itself in `fallbacks` and reads them back like everybody else (in front of
//              the per-event part, where few registers are live: the chain inlined into that part cost 36 VGPRs and a wave per SIMD); workgroup 0 waits for nobody;
//              no spin without a bound
struct InlineSegParams {
    double* seg; unsigned seg_bytes;      // the K - 1 records, and their extent (the buffer loads' bound)
    unsigned* flag; unsigned seq;         // a word on a line of its own; this hand-off's number (never 0)
    int K, polls;                         // a poll and its s_sleep(8) take about 0.25 us: the default 1024 bounds the wait at a quarter of a millisecond.
                                          // polls = 0: nobody waits (tests: every wave but workgroup 0's takes the bounded path's exit)
    unsigned* fallbacks;                  // diagnostics: waves that formed their records themselves, summed over the context's life
    int* err_next; double* knots_out;     // block 0's other duties
};
typedef __attribute__((address_space(1))) unsigned gu32;
typedef __attribute__((address_space(1))) unsigned long long gu64;
// how a lane of the inline form reads its segment record
struct InlineSegLane { __amdgpu_buffer_rsrc_t rsrc; };

// duties: workgroup 0 (the flag, and block 0's other duties of the launch this replaces); a wave that gave up waiting writes the records only
__device__ __forceinline__ void inline_seg_produce(const InlineSegParams& h, const double* __restrict__ knots, int t, bool duties)
{
    for (int sidx = t; sidx < h.K - 1; sidx += kWarpBlock) {
        double o[kSegStride];
        seg_record(sidx, knots, o);
        gu64* dst = (gu64*)(h.seg + (size_t)kSegStride * sidx);
#pragma unroll
        for (int i = 0; i < kSegStride; ++i) __hip_atomic_store(dst + i, (unsigned long long)__double_as_longlong(o[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing lane is in this one wave: drained before the flag
    if (!duties) return;
    if (t == 0) __hip_atomic_store((gu32*)h.flag, h.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == 63) h.err_next[0] = 0;
    if (h.knots_out) for (int i = t; i < 4 * h.K; i += kWarpBlock) h.knots_out[i] = knots[i];   // (for whoever reads the device copy later)
}
// true: the records are published; false: the poll budget ran out (wave-uniform either way)
__device__ __forceinline__ bool inline_seg_wait(const InlineSegParams& h)
{
    bool ready = false;
    for (int n = 0; n < h.polls; ++n) {
        const unsigned f = (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load((gu32*)h.flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (f == h.seq) { ready = true; break; }
        __builtin_amdgcn_s_sleep(8);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");     // (no instruction: the record loads stay behind the poll)
    return ready;
}

// ---- the segment records formed on the HOST (step_rule.h: prep_on_host; seg_record_rule.h: segment_records) ---------------------------------------------------
// The same steady step — clean lines, fresh texels, pixel order with the pose per event — with the K - 1 records computed by the host thread (the chain of the prep
// launch compiled for the host, while the previous Gram launch still runs) and handed to the warp kernel BY VALUE in its arguments: no launch in front, no
// producer inside, no flag.  Every one-wave workgroup copies the (K - 1) x 96 B it may index from the argument segment into LDS behind its event-word loads — into
// the bytes of the record staging tile, which is not used before the per-event part is over, so the kernel's LDS and its waves per SIMD stay what they were — and
// the per-event pose reads LDS.  Workgroup 0 takes over block 0's other duties of the launch this replaces, and leaves the records in d_seg with plain vector
// stores for whoever reads them AFTER the launch (dumps, the tile order's preparation, the solvers): nothing in the launch reads them back.
// The carrier's size: a dispatch's argument segment is 4096 B, of which the compiler keeps up to 256 B for its hidden arguments behind the explicit ones.
constexpr int kKernargBytes = 4096, kKernargHiddenBytes = 256;
struct SegHostDuties {
    double* seg_out; double* knots_out; int* err_next;   // d_seg; the device copy of the control poses; the next evaluation's status word
    int K;
    double last_knot[4];                                 // control pose K - 1 (poses 0 ... K - 2 are the records' p0)
};
constexpr int kSegByValue = (int)((kKernargBytes - kKernargHiddenBytes - sizeof(WarpParams) - sizeof(SegHostDuties)) / (kSegStride * sizeof(double)));   // records; K <= kSegByValue + 1
struct alignas(16) SegRecordsByValue { double r[kSegStride * kSegByValue]; };   // (16-B copies out of the argument segment)
static_assert(sizeof(WarpParams) + sizeof(SegHostDuties) + sizeof(SegRecordsByValue) + kKernargHiddenBytes <= kKernargBytes, "the records must fit the argument segment beside the kernel's other arguments");
static_assert(kSegByValue >= 20, "the benchmark's K = 21 must travel by value");
static_assert(kSegStride * kSegByValue <= 32 * kRecLds, "the records share the bytes of the record staging tile");
static_assert(kSegStride % 2 == 0 && sizeof(WarpParams) % 16 == 0 && sizeof(SegHostDuties) % 16 == 0, "16-B copies of the records");

__device__ __forceinline__ void host_seg_duties(const SegHostDuties& d, const SegRecordsByValue& sr, int t)
{
    typedef double v2d __attribute__((ext_vector_type(2)));
    const int n2 = (d.K - 1) * (kSegStride / 2);
    for (int k = t; k < n2; k += kWarpBlock) reinterpret_cast<v2d*>(d.seg_out)[k] = reinterpret_cast<const v2d*>(sr.r)[k];
    if (t == 63) d.err_next[0] = 0;
    if (d.knots_out) {      // (for whoever reads the device copy later; the two sources in loops of their own: each stays a load from the argument segment)
        for (int i = t; i < 4 * (d.K - 1); i += kWarpBlock) d.knots_out[i] = sr.r[kSegStride * (i >> 2) + (i & 3)];
        if (t < 4) d.knots_out[4 * (d.K - 1) + t] = d.last_knot[t];
    }
}

// What one lane knows about its measurement after the shared part.
#ifndef WARP_LATE_EP
#define WARP_LATE_EP 0     // pixel-order kernel: residual / flag stores issued after the record stores and atomics instead of in the middle
#endif
struct LaneOut {
    bool inl; uint32_t pi; int pmx, pmy; bool wr_flag;
    double jc[6], jp[6], dpx, dpy, e;
    double v0, v1, v2, v3, v4;   // the lane's terms of the per-pixel sums {w dx dx, w dx dy, w dy dy, dx we, dy we} (0 unless inlier)
};

// The per-event part shared by both kernels.  Every lane of the wave must call it (cross-lane moves inside); lane 0 of a wave
// re-warps the entry in front of the wave's 63 new ones and takes no other part.
// The event words of one lane, loaded ahead of their use: the tiled kernel walks its chunk group by group and fetches the NEXT group's
// words while it works on the current one.
struct LaneIn { uint32_t pw, bi, slot, pm; bool valid; double u; };   // pm: the entry's index in pm-order (where its residual / flag go); u: tile order (bi is then the segment)

// (the record slot is fetched here, with the event words, although only inliers use it: loaded where it is needed it would sit
// behind the lane's own stores in the in-order memory counter and every staging round would wait for the previous round's stores)
// The loads are UNCONDITIONAL (index clamped into the arrays, `valid` applied by the consumer): a load under a lane mask is waited for
// at the end of its branch, with everything issued before it — the tiled kernel's prefetch of the next group was waited for on the spot.
template <bool COMPACT, bool SEGPOSE = false>
__device__ __forceinline__ void load_event_words(const WarpParams& p, long i, bool valid, LaneIn& in)
{
    const long last = p.n_sorted - 1;               // (n_sorted >= 1 whenever a warp kernel is launched)
    const long ic = i < 0 ? 0 : (i > last ? last : i);
    in.valid = valid; in.u = 0.0;
    in.pw = stream_load(p.ev_pix + ic, COMPACT && EV_NT_LOAD); in.slot = stream_load(p.ev_slot + ic, COMPACT && EV_NT_LOAD);
    if (COMPACT) { in.pm = stream_load(p.ev_pm + ic, EV_NT_LOAD); in.u = stream_load(p.ev_u + ic, EV_NT_LOAD); in.bi = stream_load(p.ev_seg + ic, EV_NT_LOAD); }    // tile order: pm-order index, spline parameter and segment of the event's batch
    else if (SEGPOSE) { in.pm = (uint32_t)ic; in.u = p.ev_u[ic]; in.bi = p.ev_seg[ic]; }   // pixel order, pose per event: spline parameter and SEGMENT of the entry's batch
    else { in.pm = (uint32_t)ic; in.bi = stream_load(p.ev_batch + ic, EV_NT_LOAD); }
}

struct NoPrefetch { __device__ __forceinline__ void operator()() const {} };
// `prefetch` is called once, wave-uniformly, right after the texel gather has been waited for: the point of a group where nothing
// the group still needs is loaded any more.  (Loads return in order: a prefetch issued earlier sits in front of the bearing-vector,
// segment and texel gathers, and the waits for those L2 hits would pay the prefetch's HBM latency.)
// SEGPOSE (round 4; pixel order with a LARGE window): the pose is evaluated per event from its batch's spline parameter and segment record, as in the tile
// order, instead of gathered from the per-batch table — at 10 M events that table is 11 MB of 112-B records, every event pulls one or two 128-B lines of it
// past the L2 (counters: 1.37x the algorithmic bytes); u and the segment travel per entry with the event words (10 B, streamed), the K-1 segment records are a few KB.
// SEG_SRC: where a lane reads its segment record — 0 p.seg, 1 the records written inside this launch (inline_seg_*), 2 the workgroup's LDS copy of the host's records (s_seg)
template <bool DUMP, bool COMPACT = false, class PF = NoPrefetch, bool LATE_EP = false, bool SEGPOSE = false, int SEG_SRC = 0>
__device__ __forceinline__ void warp_lane(const WarpParams& p, long i, const LaneIn& in, int t, LaneOut& o, PF prefetch = PF(), const InlineSegLane* is = nullptr, const double* s_seg = nullptr)
{
    const bool valid = in.valid;
    double pm[2] = {0, 0};
    double D[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) D[k] = 0;
    uint32_t pw = 0, pol = 0;

    if (valid) {
        pw = in.pw;
        const uint32_t pix = pw & 0x1FFFFFFFu;
        pol = pw >> 31;
        const uint32_t bi = in.bi;
        const double* bv = p.lut + 3 * (size_t)pix;
        double b0, b1, b2;
        if (COMPACT) { b0 = bv[0]; b1 = bv[1]; b2 = bv[2]; }   // tile order: the bearing-vector gather is in flight while the pose is evaluated
        double R[9], J1[9];
        if (COMPACT || SEGPOSE) {   // pose per EVENT from its segment record and spline parameter (device_math.h: spline2_event)
            // (the K-1 segment records are cache-resident and fetched here, next to the bearing-vector gather whose latency is paid anyway:
            // prefetched with the event words they cost 24 VGPRs per pipeline stage)
            const uint32_t sg = bi; const double uu = in.u;
            double seg[kSegStride];
            if (SEG_SRC == 1) {   // the records were written inside this launch (inline_seg_*): sc1 loads only
                typedef unsigned int v4u __attribute__((ext_vector_type(4)));
                typedef double v2d __attribute__((ext_vector_type(2)));
                const int off = (int)(sg * (uint32_t)(kSegStride * sizeof(double)));
#pragma unroll
                for (int k = 0; k < kSegStride / 2; ++k) {
                    const v2d v = __builtin_bit_cast(v2d, (v4u)__builtin_amdgcn_raw_buffer_load_b128(is->rsrc, off + 16 * k, 0, 16));   // aux 16 = sc1
                    seg[2 * k] = v.x; seg[2 * k + 1] = v.y;
                }
            } else {
                const double2* S2 = (SEG_SRC == 2) ? reinterpret_cast<const double2*>(s_seg + kSegStride * sg)
                                                   : reinterpret_cast<const double2*>(p.seg + (size_t)kSegStride * (EMBA_ABL(p.ablate, 16) ? (sg & 1u) : sg));
                const double2 s0 = S2[0], s1 = S2[1], s2 = S2[2], s3 = S2[3], s4 = S2[4], s5 = S2[5];
                seg[0] = s0.x; seg[1] = s0.y; seg[2] = s1.x; seg[3] = s1.y; seg[4] = s2.x; seg[5] = s2.y;
                seg[6] = s3.x; seg[7] = s3.y; seg[8] = s4.x; seg[9] = s4.y; seg[10] = s5.x; seg[11] = s5.y;
            }
            double q[4];
            spline2_event<!DUMP>(seg, uu, q, J1);
            quat_to_matrix(q, R);     // rot.matrix() per event, event_pano_warper.cpp:55
        } else {
            const double2* P2 = reinterpret_cast<const double2*>(p.pose + (size_t)kPoseStride * bi);
            const double2 a0 = P2[0], a1 = P2[1], a2 = P2[2], a3 = P2[3], a4 = P2[4], a5 = P2[5], a6 = P2[6];
            const double q[4] = {a0.x, a0.y, a1.x, a1.y};
            quat_to_matrix(q, R);     // rot.matrix() per event, event_pano_warper.cpp:55
            J1[0] = a2.x; J1[1] = a2.y; J1[2] = a3.x; J1[3] = a3.y; J1[4] = a4.x; J1[5] = a4.y; J1[6] = a5.x; J1[7] = a5.y; J1[8] = a6.x;
            // (tried, round 3: J1 gathered after the projection — 18 registers fewer across it, 80 VGPRs and 6 waves / SIMD with the LDS
            // regions below aliased — 55.6 us against 50.7 at 1 M events: more resident waves do not help a kernel that runs at the memory
            // side's request rate, and the second gather is one more dependent trip)
        }
        if (!COMPACT) { b0 = bv[0]; b1 = bv[1]; b2 = bv[2]; }  // (pixel order: after the pose record — measured: 52 vs 57 us at 1 M events the other way round)
        double rb[3];
        {   // feeds round(pm): no contraction (device_math.h), the oracle's three products and two sums
#pragma clang fp contract(off)
#pragma unroll
            for (int r = 0; r < 3; ++r) rb[r] = sum3(R[3 * r] * b0, R[3 * r + 1] * b1, R[3 * r + 2] * b2);
        }
        double J23[6];
        project_chain<COMPACT && !DUMP>(rb, p.fx, p.fy, p.cx, p.cy, pm, J23);   // (the tiled kernel loops over groups: see project_angles_call)
        // dpm_ddrot_cp = J23 * [I - J1 | J1]   (model.cpp:156; J0 = I - J1, so3_spline.h:261-270)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double s0 = 0, s1 = 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double j1 = J1[3 * k + c];
                    const double j0 = ((k == c) ? 1.0 : 0.0) - j1;
                    s0 += J23[3 * r + k] * j0;
                    s1 += J23[3 * r + k] * j1;
                }
                D[6 * r + c] = s0;
                D[6 * r + c + 3] = s1;
            }
        if (DUMP) {   // (any dump pointer may be null: only what the caller asked for is produced)
            if (p.d_pm) { p.d_pm[2 * i] = pm[0]; p.d_pm[2 * i + 1] = pm[1]; }
            if (p.d_D) {
#pragma unroll
                for (int k = 0; k < 12; ++k) p.d_D[12 * i + k] = D[k];
            }
        }
    }

    // The predecessor at the same sensor pixel is the previous array element = the previous lane (kEvHasPred).
    // (Only pm travels forward; the predecessor's 2x6 Jacobian stays where it is and the two map gradients
    // travel BACKWARD instead — see j_p below — which keeps 24 VGPRs free across the long-latency texel gather.)
    const double pmp0 = dpp_shr1(pm[0]), pmp1 = dpp_shr1(pm[1]);

    bool inl = false;
    const bool cand = valid && (t >= 1) && (pw & 0x20000000u);   // kEvHasPred (never set on lead-in / halo entries)
    uint32_t pi = kInvalidPix;
    int pmx = 0, pmy = 0;
    double dpx = 0, dpy = 0, e = 0, ngx = 0, ngy = 0;   // ngx, ngy = -Gpm of an inlier (0 otherwise)
#pragma unroll
    for (int j = 0; j < 6; ++j) { o.jc[j] = 0; o.jp[j] = 0; }
    if (cand) {
        dpx = pm[0] - pmp0;
        dpy = pm[1] - pmp1;
        double dp_norm;
        {   // the outlier decision is an index-level result (who is counted in num_ev_map): no contraction, like the oracle
#pragma clang fp contract(off)
            dp_norm = sqrt(dpx * dpx + dpy * dpy);            // Eigen norm(), model.cpp:199
        }
        const double rx = round(pm[0]), ry = round(pm[1]);    // std::round, model.cpp:209-210
        // Outlier iff dp_norm > 10 (model.cpp:200).  Where the reference is undefined (non-finite dp, or a
        // rounded pixel outside the panorama read unchecked at model.cpp:213,227) the measurement is an
        // outlier as well (DESIGN.md "Defined behaviour").
        inl = (dp_norm <= p.outlier_px) && (rx >= 0.0) && (rx < (double)p.W) && (ry >= 0.0) && (ry < (double)p.H);
        if (DUMP && p.d_dp) { p.d_dp[2 * i] = dpx; p.d_dp[2 * i + 1] = dpy; }
        if (inl) {
            pmx = (int)rx; pmy = (int)ry;
            pi = (uint32_t)pmy * (uint32_t)p.W + (uint32_t)pmx;
            double gx = 0.01, gy = 0.02, gxx = 0.001, gxy = 0.002, gyy = 0.003;
            if (!EMBA_ABL(p.ablate, 4)) {
                bool use_tex = p.texel != nullptr;
                if (use_tex && p.rect_acc) {
                    int x0, y0, x1, y1;
                    texel_rect(p.rect_acc, p.W, p.H, x0, y0, x1, y1);
                    use_tex = pmx >= x0 && pmx <= x1 && pmy >= y0 && pmy <= y1;
                }
                if (use_tex) {
                    const double2* T2 = reinterpret_cast<const double2*>(p.texel + (size_t)kTexelStride * pi);
                    const double2 g = T2[0], h0 = T2[1], h1 = T2[2];
                    gx = g.x; gy = g.y; gxx = h0.x; gxy = h0.y; gyy = h1.x;
                } else {
                    hessian_at(p.Gx, p.Gy, p.H, p.W, pmx, pmy, gx, gy, gxx, gxy, gyy);
                }
            }
            const double C_pred = gx * dpx + gy * dpy;                  // model.cpp:217
            const double C_meas = 2 * ((double)pol - 0.5) * p.C_th;    // model.cpp:219
            e = C_meas - C_pred;                                        // model.cpp:221
            const double t0 = gx + (dpx * gxx + dpy * gxy);            // temp = Gpm + dp^T*G2, model.cpp:238
            const double t1 = gy + (dpx * gxy + dpy * gyy);
            if (DUMP) {
                if (p.d_Gpm) { p.d_Gpm[2 * i] = gx; p.d_Gpm[2 * i + 1] = gy; }
                if (p.d_temp) { p.d_temp[2 * i] = t0; p.d_temp[2 * i + 1] = t1; }
                if (p.d_pm_int) { p.d_pm_int[2 * i] = pmx; p.d_pm_int[2 * i + 1] = pmy; }
            } else {
#pragma unroll
                for (int j = 0; j < 6; ++j) o.jc[j] = t0 * D[j] + t1 * D[6 + j];          // model.cpp:449
                ngx = -gx; ngy = -gy;
                if (!LATE_EP) { if (EP_NT_STORE) __builtin_nontemporal_store(e, &p.e_sorted[in.pm]); else p.e_sorted[in.pm] = e; }
            }
        }
    }
    prefetch();
    o.inl = inl; o.pi = pi; o.pmx = pmx; o.pmy = pmy; o.dpx = dpx; o.dpy = dpy; o.e = e;
    if (DUMP) return;

    {   // j_p = -Gpm_k * D_{k-1} (model.cpp:459): lane k-1 owns D_{k-1}; it receives -Gpm_k from lane k, forms the 1x6 row
        // with the same two products and one sum as before, and hands the row forward.
        const double gxn = dpp_shl1(ngx), gyn = dpp_shl1(ngy);
#pragma unroll
        for (int j = 0; j < 6; ++j) o.jp[j] = dpp_shr1(gxn * D[j] + gyn * D[6 + j]);
    }
    // residual and inlier flag live at the entry's PM-ORDER index (= i in pixel order; a chain's entries are consecutive there too), so that the
    // reference-order compaction reads them in order; a lead-in / halo copy owns no pm slot of its own and writes nothing
    o.wr_flag = valid && t >= 1 && !(pw & 0x40000000u);
    if (!LATE_EP && o.wr_flag) {
        if (EP_NT_STORE) __builtin_nontemporal_store((uint8_t)(inl ? 1 : 0), &p.flag[in.pm]); else p.flag[in.pm] = inl ? 1 : 0;
    }

    // the lane's terms of the per-pixel sums (model.cpp:227 count, :426-439 A22/b2), IRLS-weighted when the cost is declared
    double v0 = dpx * dpx, v1 = dpx * dpy, v2 = dpy * dpy, v3 = dpx * e, v4 = dpy * e;   // zero unless inlier (dpx,dpy,e are)
    if (p.irls) {   // IRLS weight of the declared robust cost (same expressions as the Gram and A22-from-records kernels)
        double w;
        if (p.irls == 2) w = 1.0 / (1.0 + p.eta * e * e);                               // cauchy, model.cpp:603
        else { const double a = fabs(e); w = (a < p.eta) ? 1.0 : p.eta / a; }            // huber, :608-616
        const double ew = w * e;
        v0 = w * v0; v1 = w * v1; v2 = w * v2; v3 = dpx * ew; v4 = dpy * ew;             // A22 += w dp dp^T, b2 += dp (w e), :620-636
    }
    if (!inl) { v0 = 0; v1 = 0; v2 = 0; v3 = 0; v4 = 0; }
    o.v0 = v0; o.v1 = v1; o.v2 = v2; o.v3 = v3; o.v4 = v4;
}

// Record stores, issued COOPERATIVELY: a 128-B record is one contiguous line in HBM, so eight adjacent lanes write one record
// per wave-instruction (8 full lines per instruction) instead of every lane writing into its own line (64 partial lines per
// instruction, store-issue bound).  Only inliers have a record; they pass through a per-wave LDS tile, STAGE lanes at a time,
// COMPACTED (rank among the stage's inliers), so that every store instruction but the last of a stage is full.
template <int STAGE>
__device__ __forceinline__ void store_records(const WarpParams& p, int t, const LaneOut& o, uint32_t slot, unsigned long long inl_mask,
                                              double* s_tile /* STAGE * kRecLds doubles */, uint32_t* s_slot /* STAGE */)
{
    const int c8 = t & 7;
    // the Gram kernel's tag stream: {pano pixel, stamp} of every slot written now (one store instruction for the whole wave)
    if (p.tag && o.inl) p.tag[slot] = __hiloint2double((int)p.stamp, (int)o.pi);
#pragma unroll
    for (int st = 0; st < 64 / STAGE; ++st) {
        const unsigned long long smask = (STAGE == 64) ? inl_mask : ((inl_mask >> (STAGE * st)) & ((1ull << (STAGE & 63)) - 1ull));
        const int n_rec = __popcll(smask);
        if ((t / STAGE) == st && o.inl) {
            const int rk = __popcll(smask & ((1ull << (t % STAGE)) - 1ull));
            double2* w2 = reinterpret_cast<double2*>(s_tile + rk * kRecLds);
            w2[0] = make_double2(o.jc[0], o.jc[1]); w2[1] = make_double2(o.jc[2], o.jc[3]); w2[2] = make_double2(o.jc[4], o.jc[5]);
            w2[3] = make_double2(o.jp[0], o.jp[1]); w2[4] = make_double2(o.jp[2], o.jp[3]); w2[5] = make_double2(o.jp[4], o.jp[5]);
            w2[6] = make_double2(o.dpx, o.dpy);
            w2[7] = make_double2(o.e, __hiloint2double((int)p.stamp, (int)o.pi));
            s_slot[rk] = slot;
        }
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           // one wave: LDS ops complete in order, no barrier needed
        for (int r0 = 0; r0 < n_rec; r0 += 8) {                          // wave-uniform trip count
            const int rr = r0 + (t >> 3);
            if (rr < n_rec && !EMBA_ABL(p.ablate, 2))
            {
                typedef double v2d __attribute__((ext_vector_type(2)));
                v2d* dst = reinterpret_cast<v2d*>(p.rec + (size_t)kRecStride * (EMBA_ABL(p.ablate, 32) ? (s_slot[rr] & 8191u) : s_slot[rr])) + c8;
                const v2d val = reinterpret_cast<const v2d*>(s_tile + rr * kRecLds)[c8];
                // (non-temporal where the window's records exceed the Infinity Cache; a small window's records — the BASELINE workload: 128 MB of slots, two sets — are
                // the Gram kernel's cache hits a few microseconds later: 37.6-38.0 -> 35.3-35.8 us there)
                if (REC_NT_STORE && p.rec_nt) __builtin_nontemporal_store(val, dst);
                else *dst = val;
            }
        }
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           // tile reads done before the next stage overwrites it
    }
}

#ifndef WARP_OCC
#define WARP_OCC
#endif
template <bool DUMP, bool COMPACT, bool SEGPOSE, int SEG_SRC>
__device__ __forceinline__ void warp_residual_body(const WarpParams& p, const InlineSegParams* h, const double* knots, const SegHostDuties* hd = nullptr, const SegRecordsByValue* sr = nullptr)
{
    // One wave per workgroup, LDS operations complete in order: the record staging tile (first) and the run sums (afterwards) share
    // the same bytes, so that LDS (160 KB per CU) does not cap the resident waves below what the registers allow.
    __shared__ __attribute__((aligned(16))) double s_tile[32 * kRecLds];   // 32 staged records (half a wave) at a time: 4608 B
    static_assert(32 * kRecLds >= 64 * 6 + 32, "the run sums and their pixels must fit the staging tile");
    double* const s_acc = s_tile;                                           // per-run sums {xx xy yy bx by n} of the wave's emitting lanes, compacted (3072 B)
    uint32_t* const s_q = reinterpret_cast<uint32_t*>(s_tile + 64 * 6);     // ... and their panorama pixels (256 B)
    __shared__ uint32_t s_slot[32];                                         // record slots of the staged half's inliers

    const int t = threadIdx.x;   // == lane
    if (SEG_SRC == 1 && blockIdx.x == 0) inline_seg_produce(*h, knots, t, true);   // before anything else, and whether or not this workgroup has entries of its own
    if (SEG_SRC == 2 && blockIdx.x == 0) host_seg_duties(*hd, *sr, t);
    const long b = xcd_contiguous_block(blockIdx.x, gridDim.x);
    if (b >= p.nblk) return;  // the whole wave exits together
    const long i = b * kWarpNew + t - 1;
    const bool valid = (i >= 0) && (i < p.n_sorted);
    LaneOut o;
    LaneIn in;
    load_event_words<COMPACT, SEGPOSE>(p, i, valid, in);
    if (SEG_SRC == 2) {   // the host's records: argument segment -> LDS, behind the event-word loads just issued (one wave: LDS operations complete in order, no barrier;
                          // vector loads return in order, so these LDS writes wait for the event words as well: no extra round trip, and nothing hidden that was measured)
        typedef double v2d __attribute__((ext_vector_type(2)));
        const int n2 = (hd->K - 1) * (kSegStride / 2);       // <= kSegByValue * kSegStride / 2 (step_rule.h: prep_on_host): inside s_tile
        for (int k = t; k < n2; k += kWarpBlock) reinterpret_cast<v2d*>(s_tile)[k] = reinterpret_cast<const v2d*>(sr->r)[k];
        warp_lane<DUMP, COMPACT, NoPrefetch, (WARP_LATE_EP != 0) && !DUMP, SEGPOSE, 2>(p, i, in, t, o, NoPrefetch(), nullptr, s_tile);
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           // the record reads are done before the staging tile takes the same bytes
    } else if (SEG_SRC == 1) {
        InlineSegLane is;
        is.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)h->seg, 0, (int)h->seg_bytes, 0x00020000);    // raw buffer, 32-bit data format; loads past seg_bytes return 0
        if (blockIdx.x != 0 && !inline_seg_wait(*h)) {       // (workgroup 0 has returned from inline_seg_produce: its own stores are drained)
            inline_seg_produce(*h, knots, t, false);
            if (t == 0) atomicAdd(h->fallbacks, 1u);
        }
        warp_lane<DUMP, COMPACT, NoPrefetch, (WARP_LATE_EP != 0) && !DUMP, SEGPOSE, 1>(p, i, in, t, o, NoPrefetch(), &is);
    } else {
        warp_lane<DUMP, COMPACT, NoPrefetch, (WARP_LATE_EP != 0) && !DUMP, SEGPOSE>(p, i, in, t, o);
    }
    if (DUMP) return;
    const bool inl = o.inl;
    const uint32_t pi = o.pi;
    const unsigned long long inl_mask = __ballot(inl);

    // Records first, per-pixel sums second: loads, stores and atomics share one in-order counter per wave, so anything that waits
    // for a load issued after the atomics would wait for the atomics' round trip to the memory side too.
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) (event words, pose, texels, slot: long done; the residual / flag stores: two small ones); the builtin, so that the
                                          // compiler knows nothing is pending and does not wait again inside the staging rounds, behind their own stores
    store_records<32>(p, t, o, in.slot, inl_mask, s_tile, s_slot);

    // Per-pixel sums.  Consecutive events of a sensor pixel often land on the SAME panorama
    // pixel (dense streams: the camera moves a fraction of a pixel between them), and every atomic costs one memory-side request
    // whatever it carries, so runs of adjacent lanes with equal pixel are summed first (segmented inclusive scan over the wave,
    // heads where the pixel changes) and only the last lane of a run emits: one int add of the run length, five fp64 adds.
    double v0 = o.v0, v1 = o.v1, v2 = o.v2, v3 = o.v3, v4 = o.v4;
    int run_n = inl ? 1 : 0;
    const uint32_t key = inl ? pi : (kInvalidPix - (uint32_t)t);                     // non-inliers never join a run
    const bool head = (t == 0) || (key != (uint32_t)dpp_shr1((int)key));
    const bool cont = inl && !head;                                                  // continues its neighbour's run
    if (__ballot(cont)) {   // (wave-uniform) otherwise every run is one lane long
        // Round 4: 91 % of the waves have a run, nearly all of them runs of TWO lanes (5.5 % of the inliers continue a neighbour, almost none a
        // neighbour that itself continues one): one step of row moves (DPP, no LDS) instead of the six-step segmented scan — 71 ds_bpermute and
        // ~100 vector instructions per wave — which stays for the waves that do hold a longer run.  Same sums in the same order.
        const bool deep = cont && (dpp_shr1(cont ? 1 : 0) != 0);                     // the lane in front continues a run too: three or more
        if (__ballot(deep)) {
            int flag = head ? 1 : 0;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int f_up = __shfl_up(flag, d), n_up = __shfl_up(run_n, d);
                const double a0 = __shfl_up(v0, d), a1 = __shfl_up(v1, d), a2 = __shfl_up(v2, d), a3 = __shfl_up(v3, d), a4 = __shfl_up(v4, d);
                if (t >= d && !flag) { v0 += a0; v1 += a1; v2 += a2; v3 += a3; v4 += a4; run_n += n_up; flag = f_up; }
            }
        } else {
            const int n_up = dpp_shr1(run_n);
            const double a0 = dpp_shr1(v0), a1 = dpp_shr1(v1), a2 = dpp_shr1(v2), a3 = dpp_shr1(v3), a4 = dpp_shr1(v4);
            if (cont) { v0 += a0; v1 += a1; v2 += a2; v3 += a3; v4 += a4; run_n += n_up; }
        }
    }
    const int head_next = dpp_shl1(head ? 1 : 0);                                    // (cross-lane reads stay in uniform control flow)
    const bool emit = inl && ((t == 63) || (head_next != 0));                        // last lane of its run
    const unsigned long long emit_mask = __ballot(emit);
    // The warp kernel runs at the chip's memory-side atomic REQUEST rate (rocprofv3: TCC_EA0_ATOMIC x 64 B / kernel time was
    // 1.0 of the ~1.3 TB/s the chip sustains), so every measurement costs exactly ONE atomic request: the count of a pixel
    // (model.cpp:227) rides as a sixth double in the same 64-B accumulator line as its five A22/b2 sums.  The int32 count map
    // only receives a plain store of a non-zero MARKER here ("this pixel was touched"); emba_post_warp_a_kernel (or
    // emba_count_materialise_kernel when someone needs the map earlier) replaces markers by the counts from the lines.
    // Run sums are compacted through LDS and sent 10 pixels = 60 lanes per atomic instruction.
    if (emit && !EMBA_ABL(p.ablate, 1)) p.count[pi] = p.marker;
    {
        const int n_emit = __popcll(emit_mask);
        if (emit) {
            const int rk = __popcll(emit_mask & ((1ull << t) - 1ull));
            double* a = s_acc + rk * 6;
            a[0] = v0; a[1] = v1; a[2] = v2; a[3] = v3; a[4] = v4; a[5] = (double)run_n;
            s_q[rk] = pi;
        }
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           // one wave: LDS ops complete in order, no barrier needed
        const int r10 = t / 6, comp = t - 6 * r10;
        for (int g = 0; g < n_emit; g += 10) {                           // wave-uniform trip count
            const int k = g + r10;
            if (t < 60 && k < n_emit && !EMBA_ABL(p.ablate, 8))
                atomicAdd(p.pixacc + (size_t)kPixAccStride * s_q[k] + comp, s_acc[6 * k + comp]);
        }
    }
    if (WARP_LATE_EP) {   // residual and inlier flag at the entry's pm-order index, last: nothing in this wave waits for them
        if (inl) { if (EP_NT_STORE) __builtin_nontemporal_store(o.e, &p.e_sorted[in.pm]); else p.e_sorted[in.pm] = o.e; }
        if (o.wr_flag) { if (EP_NT_STORE) __builtin_nontemporal_store((uint8_t)(inl ? 1 : 0), &p.flag[in.pm]); else p.flag[in.pm] = inl ? 1 : 0; }
    }
}

template <bool DUMP, bool COMPACT = false, bool SEGPOSE = false>
__global__ __launch_bounds__(kWarpBlock) WARP_OCC void emba_warp_residual_kernel(WarpParams p)
{
    warp_residual_body<DUMP, COMPACT, SEGPOSE, 0>(p, nullptr, nullptr);
}
// pixel order, pose per event, the segment records formed by workgroup 0 of this launch (inline_seg_*)
// (five waves per SIMD like the form it replaces: the producer's chain — so3_log, sin, cos: 128 VGPRs on its own — spills 144 B per lane in the two places that run
// it; the per-event part fits as before)
#ifndef EMBA_INLINE_WARP_OCC
#define EMBA_INLINE_WARP_OCC __attribute__((amdgpu_waves_per_eu(5, 5)))
#endif
__global__ __launch_bounds__(kWarpBlock) EMBA_INLINE_WARP_OCC void emba_warp_residual_inline_kernel(WarpParams p, InlineSegParams h, InlineKnots kn)
{
    warp_residual_body<false, false, true, 1>(p, &h, kn.q);
}
// pixel order, pose per event, the segment records formed by the host and carried in the arguments (SegRecordsByValue)
__global__ __launch_bounds__(kWarpBlock) WARP_OCC void emba_warp_residual_hostseg_kernel(WarpParams p, SegHostDuties d, SegRecordsByValue sr)
{
    warp_residual_body<false, false, true, 2>(p, nullptr, nullptr, &d, &sr);
}

// Tile order: blockIdx -> chunk of one panorama bin's events (ChunkDesc).  The workgroup's waves take the chunk's 63-entry groups
// round-robin; inlier measurements whose pixel lies inside the LDS tile (under the poses the order was built from: all of them, with a reserve of a few pixels on every side — trial poses
// of an LM loop move events by a few pixels) add their six terms with LDS atomics, the few outside go to HBM directly; at the end
// every touched pixel of the tile costs ONE atomic request to its 64-B accumulator line and one marker store.
template <int kTileW, int kTileH>
__global__ __launch_bounds__(kTileWaves * 64) __attribute__((amdgpu_waves_per_eu(TILE_OCC, TILE_OCC))) void emba_warp_tiled_kernel(WarpParams p)
{
    constexpr int kTilePx = kTileW * kTileH;
    __shared__ double s_sum[6][kTilePx];                                                  // SoA: plane k = k-th term of every tile pixel
    __shared__ __attribute__((aligned(16))) double s_tile[kTileWaves][kTileRecStage * kRecLds];
    __shared__ uint32_t s_slot[kTileWaves][kTileRecStage];
    __shared__ uint16_t s_list[kTileWaves][64];

    const int tid = threadIdx.x, t = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // One chunk per workgroup; the list is sorted longest first and walked in grid order (chunks_linear).  (Round 6 tried the other way round — the entry list, in
    // tile order, cut into one EQUAL share per workgroup slot of the chip, a workgroup working through the pieces of tiles in its share: 2 M events 113 -> 145 us,
    // 3 M 160 -> 194, city 495 -> 538: a piece of G groups takes ceil(G / 8) rounds of the workgroup's eight waves whatever its size, and with two or three pieces
    // per share the slowest workgroup — the kernel's end — is the one whose pieces round worst; profiles/r06_share_form_sweep.txt.)
    const long c = p.chunks_linear ? (long)blockIdx.x : xcd_contiguous_block(blockIdx.x, gridDim.x);
    if (c >= p.n_chunks) return;      // (block-uniform)
    for (int k = tid; k < 6 * kTilePx; k += kTileWaves * 64) (&s_sum[0][0])[k] = 0.0;
    __syncthreads();
    {
        const ChunkDesc ch = p.chunks[c];
        {
            const long begin = ch.begin, end = ch.end;
            constexpr long kStep = (long)kWarpNew * kTileWaves;
            // Software pipeline over the wave's groups.  Loads, stores and atomics of a wave share ONE in-order counter (vmcnt): waiting
            // for a load means waiting for everything issued before it.  Each iteration therefore: (1) works on group g from registers
            // — its waits are for its own bearing-vector / segment / texel gathers (cache hits), behind which nothing slow is queued;
            // (2) once the texels are here issues the event words, spline parameters and record slots of group g+1 (HBM streams), which
            // have the group's remaining arithmetic and LDS atomics to arrive; (3) waits for everything once and rotates the registers;
            // (4) issues the record stores last.
            // Before: a vmcnt(0) per staging round and one at the loop head = ~15 us per group, 67 % of wave time waiting.
            // (Round 6, measured and dropped: the NEXT group's bearing-vector / segment gathers issued in front of this group's record stores, the stores in a
            // static number — lanes without a record writing to a trash line — so that the next group's first wait is vmcnt(8) and does not include the stores'
            // acknowledgements: the ISA did what was intended and the kernel got SLOWER, city 490 -> 537 us, 10 M 461 -> 469, 40 M 1784 -> 1832, 3 M equal
            // (profiles/r06_early_gather_ab.txt; 112 instead of 101 VGPRs).  The acknowledgement wait is not what the wave loses: by ablation the record stores
            // cost 14-21 % of the kernel, a third to a half of that with the stores going to a cache-resident window — issue and drain, not the wait.)
            LaneIn cur, nxt;
            {
                const long g0 = begin + (long)kWarpNew * wv;
                const long i0 = g0 + t - 1;
                load_event_words<true>(p, i0, g0 < end && i0 >= 0 && i0 < end, cur);
                __builtin_amdgcn_s_waitcnt(0x0F70);   // (so that `cur` is known to be loaded on BOTH ways into the loop: see (3))
            }
#pragma unroll 1
            for (long g0 = begin + (long)kWarpNew * wv; g0 < end; g0 += kStep) {   // wave-uniform
                const long i = g0 + t - 1;
                auto prefetch = [&]() { const long i1 = i + kStep; load_event_words<true>(p, i1, g0 + kStep < end && i1 < end, nxt); };
                LaneOut o;
                warp_lane<false, true>(p, i, cur, t, o, prefetch);
                const unsigned long long inl_mask = __ballot(o.inl);
                bool outside = false;
                if (o.inl) {
                    const int lx = o.pmx - ch.x0, ly = o.pmy - ch.y0;
                    outside = !(lx >= 0 && lx < kTileW && ly >= 0 && ly < kTileH);
                    if (!outside) {
                        const int q = ly * kTileW + lx;
                        if (!EMBA_ABL(p.ablate, 8)) {
                            atomicAdd(&s_sum[0][q], o.v0); atomicAdd(&s_sum[1][q], o.v1); atomicAdd(&s_sum[2][q], o.v2);
                            atomicAdd(&s_sum[3][q], o.v3); atomicAdd(&s_sum[4][q], o.v4); atomicAdd(&s_sum[5][q], 1.0);
                        }
                    } else {   // moved out of the tile since the order was built: still correct, just not aggregated
                        double* a = p.pixacc + (size_t)kPixAccStride * o.pi;
                        p.count[o.pi] = p.marker;
                        atomicAdd(a + 0, o.v0); atomicAdd(a + 1, o.v1); atomicAdd(a + 2, o.v2); atomicAdd(a + 3, o.v3); atomicAdd(a + 4, o.v4); atomicAdd(a + 5, 1.0);
                    }
                }
                {   // how many: the host re-bins the window for the next evaluation when the trajectory has drifted away from the one the order was built for
                    const unsigned long long om = __ballot(outside);
                    if (om && t == 0 && p.err) atomicAdd(p.err, 2 * (int)__popcll(om));
                }
                const uint32_t slot = cur.slot;
                __builtin_amdgcn_s_waitcnt(0x0F70);   // (3) vmcnt(0): the prefetched words are in.  The builtin, not inline asm: the compiler's own wait-count bookkeeping must
                                                      // know it, or it waits again at the next iteration's first use of `cur` — behind the record stores issued below
                cur = nxt;
                __builtin_amdgcn_sched_barrier(0);
                store_records<kTileRecStage>(p, t, o, slot, inl_mask, s_tile[wv], s_slot[wv]);   // (4)
            }
        }
        __syncthreads();
        // flush: wave by wave over the tile's pixels; touched ones are listed (LDS) and sent 10 pixels = 60 lanes per atomic instruction
        for (int q0 = wv * 64; q0 < kTilePx; q0 += kTileWaves * 64) {
            const int q = q0 + t;
            const bool touched = q < kTilePx && s_sum[5][q] > 0.0;
            const unsigned long long m = __ballot(touched);
            if (!m) continue;
            if (touched) s_list[wv][__popcll(m & ((1ull << t) - 1ull))] = (uint16_t)q;
            __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const int n_emit = __popcll(m);
            const int r10 = t / 6, comp = t - 6 * r10;
            for (int g = 0; g < n_emit; g += 10) {
                const int k = g + r10;
                if (t < 60 && k < n_emit) {
                    const int qq = s_list[wv][k];
                    const int gy = ch.y0 + qq / kTileW, gx = ch.x0 + qq % kTileW;
                    const size_t pi = (size_t)gy * p.W + gx;
                    if (comp == 0 && !EMBA_ABL(p.ablate, 1)) p.count[pi] = p.marker;
                    if (!EMBA_ABL(p.ablate, 8)) atomicAdd(p.pixacc + (size_t)kPixAccStride * pi + comp, s_sum[comp][qq]);
                }
            }
            __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }
}

inline void launch_warp_tiled(int shape, dim3 grid, hipStream_t s, const WarpParams& p)
{
    switch (shape) {
    case 1: hipLaunchKernelGGL((emba_warp_tiled_kernel<kTileShapes[1].tw, kTileShapes[1].th>), grid, dim3(kTileWaves * 64), 0, s, p); break;
    case 2: hipLaunchKernelGGL((emba_warp_tiled_kernel<kTileShapes[2].tw, kTileShapes[2].th>), grid, dim3(kTileWaves * 64), 0, s, p); break;
    case 3: hipLaunchKernelGGL((emba_warp_tiled_kernel<kTileShapes[3].tw, kTileShapes[3].th>), grid, dim3(kTileWaves * 64), 0, s, p); break;
    default: hipLaunchKernelGGL((emba_warp_tiled_kernel<kTileShapes[0].tw, kTileShapes[0].th>), grid, dim3(kTileWaves * 64), 0, s, p); break;
    }
}

// ------------------------------------------------------------------------------------------------
// Exclusive scan of per-block counts (single block, sequential over 1024-wide tiles).
// out[i] = sum_{j<i} in[j]; total[0] = sum of all.
// ------------------------------------------------------------------------------------------------
// out[i] = sum_{j<i} in[j] for one 256-thread block, 16 consecutive entries per thread and tile.
__device__ __forceinline__ void block_scan_256(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, long n,
                                               uint32_t* __restrict__ total, int* __restrict__ total_host,
                                               const int* __restrict__ err_dev, int* __restrict__ err_host)
{
    // (callable from blocks of >= 256 threads: every thread must call it, threads >= 256 only keep the barriers company)
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_carry;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const bool worker = t < 256;
    if (t == 0) s_carry = 0;
    __syncthreads();
    for (long base = 0; base < n; base += 4096) {
        const long i = base + 16 * t;
        uint32_t v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = (worker && i + k < n) ? in[i + k] : 0;
        uint32_t mine = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) mine += v[k];
        uint32_t x = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (worker && lane == 63) s_wave[wv] = x;
        __syncthreads();
        uint32_t woff = 0;
        for (int w = 0; w < wv && w < 4; ++w) woff += s_wave[w];
        const uint32_t carry = s_carry;
        uint32_t run = carry + woff + x - mine;
#pragma unroll
        for (int k = 0; k < 16; ++k) { if (worker && i + k < n) out[i + k] = run; run += v[k]; }
        __syncthreads();
        if (t == 255) s_carry = carry + woff + x;
        __syncthreads();
    }
    if (t == 0) {
        total[0] = s_carry;
        if (total_host) total_host[0] = (int)s_carry;       // pinned, device-visible host word: no copy node needed
        if (err_host) err_host[0] = err_dev[0];
    }
}

__global__ __launch_bounds__(256) void emba_scan_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                         long n, uint32_t* __restrict__ total, int* __restrict__ total_host,
                                                         const int* __restrict__ err_dev, int* __restrict__ err_host)
{
    block_scan_256(in, out, n, total, total_host, err_dev, err_host);
}

// Block-wide exclusive rank of a flag among 256 threads (4 waves) via ballots.
__device__ __forceinline__ uint32_t block_rank_256(bool f, uint32_t* s_w /*[4]*/)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(f);
    const uint32_t within = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[wv] = __popcll(m);
    __syncthreads();
    uint32_t off = 0;
    for (int w = 0; w < wv; ++w) off += s_w[w];
    return off + within;
}

// Residual compaction into the reference's order (model.cpp:221,256): sensor pixel major, then time = "pm-order".  The warp
// kernels leave residual and inlier flag per entry of the DEVICE order; perm maps a pm-order index to its device entry
// (nullptr: the device order IS the pm-order; 0xFFFFFFFF: a halo entry, never a measurement).  Blocks of kFlagBlk pm entries,
// four consecutive ones per thread: count -> scan over blocks -> compact.
constexpr int kFlagBlk = 1024;

__device__ __forceinline__ uint32_t flag_quad(long i0, long n_pm, const uint8_t* __restrict__ flag, const uint32_t* __restrict__ perm, uint32_t* j_out)
{
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long i = i0 + k;
        uint32_t j = 0xFFFFFFFFu;
        if (i < n_pm) j = perm ? perm[i] : (uint32_t)i;
        j_out[k] = j;
        if (j != 0xFFFFFFFFu && flag[j]) m |= 1u << k;
    }
    return m;
}

// (round 6) fsup: the counts of kFlagSup consecutive blocks summed — 64 K pm entries per word —, so that a tail block of the Gram launch (ep_tail_block) finds the
// inliers in front of it from <= 63 block counts + one word per 64 K entries in front of those (1526 words at 100 M events) whatever the window's length.
// Every super-count has a 64-B line of its own (kFlagSupStride words apart) and 64 adders: atomics on one LINE are served one after the other at the memory side —
// with the super-counts packed (977 adds to one line at 1 M events, whether into one word or sixteen) launch A took 18.0 instead of 8.5 us.
constexpr int kFlagSup = 64;
constexpr int kFlagSupStride = 16;
__device__ __forceinline__ void flag_count_block(long blk, const uint8_t* __restrict__ flag, const uint32_t* __restrict__ perm, long n_pm,
                                                 uint32_t* __restrict__ fblk_cnt, uint32_t* __restrict__ fsup = nullptr)
{
    __shared__ uint32_t s_w[4];
    uint32_t j[4];
    uint32_t c = __popc(flag_quad(blk * kFlagBlk + 4 * threadIdx.x, n_pm, flag, perm, j));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t n = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
        fblk_cnt[blk] = n;
        if (fsup && n) atomicAdd(fsup + (blk / kFlagSup) * kFlagSupStride, n);
    }
}

__device__ __forceinline__ void compact_ep_block(long blk, const double* __restrict__ e_sorted, const uint8_t* __restrict__ flag,
                                                 const uint32_t* __restrict__ perm, const uint32_t* __restrict__ fblk_off, long n_pm,
                                                 double* __restrict__ ep, int32_t* __restrict__ inl_idx)
{
    __shared__ uint32_t s_w[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t j[4];
    const uint32_t m = flag_quad(blk * kFlagBlk + 4 * threadIdx.x, n_pm, flag, perm, j);
    const uint32_t mine = __popc(m);
    uint32_t x = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o); if (lane >= o) x += y; }
    if (lane == 63) s_w[wv] = x;
    __syncthreads();
    uint32_t k = fblk_off[blk] + x - mine;
    for (int w = 0; w < wv; ++w) k += s_w[w];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (j[q] == 0xFFFFFFFFu) continue;
        if (m & (1u << q)) { ep[k] = e_sorted[j[q]]; if (inl_idx) inl_idx[j[q]] = (int32_t)k; ++k; }
        else if (inl_idx) inl_idx[j[q]] = -1;
    }
}

__global__ __launch_bounds__(256) void emba_flag_count_kernel(const uint8_t* __restrict__ flag, const uint32_t* __restrict__ perm, long n_pm,
                                                              uint32_t* __restrict__ fblk_cnt)
{
    flag_count_block(blockIdx.x, flag, perm, n_pm, fblk_cnt);
}

__global__ __launch_bounds__(256) void emba_compact_ep_kernel(const double* __restrict__ e_sorted, const uint8_t* __restrict__ flag,
                                                              const uint32_t* __restrict__ perm, const uint32_t* __restrict__ fblk_off,
                                                              long n_pm, double* __restrict__ ep, int32_t* __restrict__ inl_idx)
{
    compact_ep_block(blockIdx.x, e_sorted, flag, perm, fblk_off, n_pm, ep, inl_idx);
}

// Sensor pixel of every inlier measurement, in ep order (the pm-order IS sensor pixel major, then time): what a multi-GPU host needs to
// merge the ranks' residual vectors into the reference's order.
__global__ void emba_inlier_pix_kernel(const uint32_t* __restrict__ pm_pix, const uint8_t* __restrict__ flag, const int32_t* __restrict__ inl_idx, long n_pm,
                                       uint32_t* __restrict__ out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pm || !flag[i]) return;
    out[inl_idx[i]] = pm_pix[i] & 0x1FFFFFFFu;
}

// ... and where every sensor pixel's residuals begin in the rank's ep: starts[p] = number of inliers at sensor pixels < p (starts[S] = all), from the list above
// (ascending).  Thread i <= m fills the pixels (px[i-1], px[i]] — the pixels without inliers in between take the same start.  A multi-GPU host places a rank's
// residuals pixel block by pixel block from these S + 1 words instead of one word per residual (round 6).
__global__ void emba_pix_starts_kernel(const uint32_t* __restrict__ px, long m, uint32_t S, uint32_t* __restrict__ starts)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    const uint32_t lo = (i == 0) ? 0u : px[i - 1] + 1u;
    const uint32_t hi = (i == m) ? S : (px[i] < S ? px[i] : S);
    for (uint32_t q = lo; q <= hi && q <= S; ++q) starts[q] = (uint32_t)i;
}

// Caller-supplied residuals (the `ep` argument of formNormalEq, model.cpp:421): scatter into the records.
__global__ void emba_override_ep_kernel(const double* __restrict__ ep_ext, const uint8_t* __restrict__ flag,
                                        const int32_t* __restrict__ inl_idx, const uint32_t* __restrict__ ev_slot, const uint32_t* __restrict__ ev_pix,
                                        const uint32_t* __restrict__ ev_pm, long n_sorted, double* __restrict__ rec, double* __restrict__ e_sorted)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sorted || (ev_pix[i] & 0x40000000u)) return;      // (lead-in / halo copies are nobody's measurement)
    const long f = ev_pm ? (long)ev_pm[i] : i;                   // residual, flag and inlier number live at the pm-order index
    if (!flag[f]) return;
    const double e = ep_ext[inl_idx[f]];
    rec[(size_t)kRecStride * ev_slot[i] + 14] = e;
    e_sorted[f] = e;
}

// ------------------------------------------------------------------------------------------------
// a8: active set (count >= thres) in ascending panorama index (model.cpp:325-344, 371-377).
// 2048 pixels per block, 8 consecutive pixels per thread (two 16-B loads), so a 1024x2048 panorama needs 1024 block
// counts and the scan between the two kernels is a single tile.
// ------------------------------------------------------------------------------------------------
constexpr int kActivePix = 2048;

__device__ __forceinline__ uint32_t active_mask8(const int32_t* __restrict__ count, long p0, long npix, int thres, uint32_t* touched = nullptr)
{   // touched (optional): which of the 8 pixels have a non-zero count
    uint32_t m = 0, tm = 0;
    if (p0 + 8 <= npix) {
        const int4 a = *reinterpret_cast<const int4*>(count + p0), b = *reinterpret_cast<const int4*>(count + p0 + 4);
        m = (a.x >= thres) | ((a.y >= thres) << 1) | ((a.z >= thres) << 2) | ((a.w >= thres) << 3) | ((b.x >= thres) << 4) |
            ((b.y >= thres) << 5) | ((b.z >= thres) << 6) | ((b.w >= thres) << 7);
        tm = (a.x != 0) | ((a.y != 0) << 1) | ((a.z != 0) << 2) | ((a.w != 0) << 3) | ((b.x != 0) << 4) | ((b.y != 0) << 5) | ((b.z != 0) << 6) | ((b.w != 0) << 7);
    } else {
        for (int k = 0; k < 8; ++k) if (p0 + k < npix) { const int c = count[p0 + k]; if (c >= thres) m |= 1u << k; if (c) tm |= 1u << k; }
    }
    if (touched) *touched = tm;
    return m;
}

// The same over a RAW count map (markers left by the warp kernel): a touched pixel's count is the sixth double of its accumulator
// line; the counts are written back, which turns the map into the num_ev_map of model.cpp:227 for everyone downstream.
__device__ __forceinline__ uint32_t materialise_mask8(int32_t* __restrict__ count, const double* __restrict__ pixacc, long p0, long npix, int thres,
                                                      int32_t marker, uint32_t* touched = nullptr, int* c_out = nullptr)
{
    // entry == marker: touched by THIS evaluation -> its count from the accumulator line; anything else that is not zero is what an earlier
    // evaluation left behind (counts, or markers nobody asked about) -> zero.  The map needs no clearing pass between evaluations.
    int c[8];
    const bool full = p0 + 8 <= npix;
    if (full) {
        const int4 a = *reinterpret_cast<const int4*>(count + p0), b = *reinterpret_cast<const int4*>(count + p0 + 4);
        c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w; c[4] = b.x; c[5] = b.y; c[6] = b.z; c[7] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = (p0 + k < npix) ? count[p0 + k] : 0;
    }
    int any = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) any |= c[k];
    if (any) {
        // (unconditional loads — an entry that is not this evaluation's marker re-reads the thread's first pixel: eight loads under eight lane
        // masks are eight dependent round trips for a lane in the middle of the footprint)
        double n8[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) n8[k] = pixacc[(size_t)kPixAccStride * (p0 + ((c[k] == marker) ? k : 0)) + 5];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = (c[k] == marker) ? (int)n8[k] : 0;
        if (full) {
            *reinterpret_cast<int4*>(count + p0) = make_int4(c[0], c[1], c[2], c[3]);
            *reinterpret_cast<int4*>(count + p0 + 4) = make_int4(c[4], c[5], c[6], c[7]);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) if (p0 + k < npix) count[p0 + k] = c[k];
        }
    }
    uint32_t m = 0, tm = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { m |= (uint32_t)(c[k] >= thres) << k; tm |= (uint32_t)(c[k] != 0) << k; }
    if (touched) *touched = tm;
    if (c_out) {
#pragma unroll
        for (int k = 0; k < 8; ++k) c_out[k] = c[k];
    }
    return m;
}

__global__ __launch_bounds__(256) void emba_count_materialise_kernel(int32_t* __restrict__ count, const double* __restrict__ pixacc, long npix, int32_t marker)
{
    (void)materialise_mask8(count, pixacc, ((long)blockIdx.x * 256 + threadIdx.x) * 8, npix, 1, marker);
}

__device__ __forceinline__ void active_count_block(long blk, const int32_t* __restrict__ count, long npix, int thres,
                                                   uint32_t* __restrict__ blk_cnt, int32_t* raw_count = nullptr, const double* pixacc = nullptr,
                                                   uint8_t* __restrict__ active_bits = nullptr, int* __restrict__ blk_rect = nullptr, int W = 1, int32_t marker = 0,
                                                   uint16_t* __restrict__ seg = nullptr, double* __restrict__ clear_inactive = nullptr,
                                                   const uint8_t* __restrict__ global_u8 = nullptr)
{
    // global_u8 (a rank of a sharded window, round 5): activity — count >= thres, model.cpp:333,409 — is a property of the GLOBAL counts, which the host has
    // all-reduced as saturated bytes (exchange 1); `count` then holds THIS rank's materialised counts and only says which pixels the rank touched (the lines
    // to clear, the texel rectangle).  A pixel can be active without a local measurement: its line is zero and its row of A22 | b2 comes from the others.
    // seg (the resident one-GPU step): the unit's active pixels, ascending, as offsets inside the unit at seg[blk * kActivePix + rank] — the
    // gather that follows (active_gather_block) then works from lists, balanced over the whole grid, instead of sweeping the count map again.
    // clear_inactive (same step): the accumulator lines of touched pixels that did NOT become active are zeroed here (their count has just been
    // read; nobody else reads them), the active ones by the gather, so that the next evaluation starts on clean lines without a clearing pass.
    __shared__ uint32_t s_w[4];
    const long p0 = blk * kActivePix + 8 * threadIdx.x;
    uint32_t tm = 0;
    uint32_t m8 = raw_count ? materialise_mask8(raw_count, pixacc, p0, npix, thres, marker, &tm) : active_mask8(count, p0, npix, thres, &tm);
    if (global_u8) {
        m8 = 0;
        if (p0 + 8 <= npix) {
            const uint2 g = *reinterpret_cast<const uint2*>(global_u8 + p0);
#pragma unroll
            for (int k = 0; k < 4; ++k) { m8 |= (uint32_t)((int)((g.x >> (8 * k)) & 255u) >= thres) << k; m8 |= (uint32_t)((int)((g.y >> (8 * k)) & 255u) >= thres) << (4 + k); }
        } else {
            for (int k = 0; k < 8; ++k) if (p0 + k < npix && (int)global_u8[p0 + k] >= thres) m8 |= 1u << k;
        }
    }
    if (active_bits && p0 < npix) active_bits[p0 >> 3] = (uint8_t)m8;
    if (blk_rect) {   // bounding box of the pixels THIS evaluation touched, per block; the active-write kernel's last block reduces them
        __shared__ int s_box[4][4];     // into the rectangle the next evaluation packs its texels in
        int xmin = 0x7FFFFFFF, ymin = 0x7FFFFFFF, xmax = -1, ymax = -1;
        if (tm) {
            if ((W & 7) == 0) {      // the thread's 8 pixels lie in one row: one division, the ends from the lowest / highest touched bit
                const int y = (int)(p0 / W), x = (int)(p0 - (long)y * W);
                xmin = x + (__ffs((int)tm) - 1); xmax = x + (31 - __clz((int)tm)); ymin = y; ymax = y;
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (tm & (1u << k)) { const int idx = (int)(p0 + k), y = idx / W, x = idx - y * W; xmin = min(xmin, x); xmax = max(xmax, x); ymin = min(ymin, y); ymax = max(ymax, y); }
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            xmin = min(xmin, __shfl_xor(xmin, o)); ymin = min(ymin, __shfl_xor(ymin, o));
            xmax = max(xmax, __shfl_xor(xmax, o)); ymax = max(ymax, __shfl_xor(ymax, o));
        }
        if ((threadIdx.x & 63) == 0) { int* b = s_box[threadIdx.x >> 6]; b[0] = xmin; b[1] = ymin; b[2] = xmax; b[3] = ymax; }
        __syncthreads();
        if (threadIdx.x == 0) {
            int4 r;
            r.x = min(min(s_box[0][0], s_box[1][0]), min(s_box[2][0], s_box[3][0]));
            r.y = min(min(s_box[0][1], s_box[1][1]), min(s_box[2][1], s_box[3][1]));
            r.z = max(max(s_box[0][2], s_box[1][2]), max(s_box[2][2], s_box[3][2]));
            r.w = max(max(s_box[0][3], s_box[1][3]), max(s_box[2][3], s_box[3][3]));
            reinterpret_cast<int4*>(blk_rect)[blk] = r;
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t mine = __popc(m8);
    uint32_t x = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o); if (lane >= o) x += y; }
    if (lane == 63) s_w[wv] = x;
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blk] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
    if (seg) {
        uint32_t r = x - mine;
        for (int w = 0; w < wv; ++w) r += s_w[w];
        uint16_t* sg = seg + (size_t)blk * kActivePix;
#pragma unroll
        for (int k = 0; k < 8; ++k) if (m8 & (1u << k)) sg[r++] = (uint16_t)(8 * threadIdx.x + k);
    }
    if (clear_inactive) {
        const uint32_t z = tm & ~m8;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (z & (1u << k)) {
                double2* q = reinterpret_cast<double2*>(clear_inactive + (size_t)kPixAccStride * (p0 + k));
                q[0] = make_double2(0, 0); q[1] = make_double2(0, 0); q[2] = make_double2(0, 0);
            }
    }
}

__global__ __launch_bounds__(256) void emba_active_count_kernel(const int32_t* __restrict__ count, long npix, int thres,
                                                                uint32_t* __restrict__ blk_cnt)
{
    active_count_block(blockIdx.x, count, npix, thres, blk_cnt);
}

// The two small post-warp chains (residual compaction: count -> scan -> compact; active set: count -> scan -> write) are
// independent of each other, so their stages share launches ("heterogeneous" kernels):
//   A = {active-count blocks | inlier-flag-count blocks}, then the active-write blocks, which take their own prefix over A's per-block counts
//   and publish the totals (no scan launch in between; the residual compaction itself runs only when the host asks for `ep`)
struct PostWarpParams {
    const int32_t* count; long npix; int thres; uint32_t* ablk_cnt; uint32_t* ablk_off; long n_ablk; uint32_t* total_P; int* total_P_host;
    uint32_t* fblk_cnt; uint32_t* fblk_off; long n_fblk; const uint32_t* perm; long n_pm; uint32_t* total_inl; int* total_inl_host; const int* err_dev; int* err_host;
    const double* e_sorted; const uint8_t* flag; double* ep; int32_t* inl_idx;
    int seq; int* seq_host;   // step sequence number, written to pinned host memory AFTER the counts (two words: [0] behind P, [1] behind the inlier count): the host may poll them instead of waiting for the stream
    int32_t* raw_count; const double* pixacc; int32_t marker;   // non-null: the count map still holds the warp kernel's markers (count_marker of its stamp); launch A materialises it
    uint8_t* active_bits; double* pack_head; long head_len;   // non-null: launch A also writes the 1-bit activity map and clears A11 | b1 (the Gram kernel then
                                                              // depends on launch A only)
    int* blk_rect; int W;                                     // non-null: per-block bounding boxes of the touched pixels (-> the next evaluation's texel rectangle)
    uint16_t* seg; double* clear_inactive;                    // the resident one-GPU step (active_count_block): per-unit active lists; zero the lines of touched, inactive pixels
    const uint8_t* global_u8;                                 // a sharded window's rank: activity from the all-reduced saturated byte counts (active_count_block)
    uint32_t* fsup; uint32_t* fsup_next; long n_sup;          // non-null: the flag-count blocks also sum into this step's super-counts (flag_count_block); block 0 zeroes the NEXT step's
};

struct ActiveWriteParams {
    const int32_t* count; long npix; int thres; const uint32_t* blk_off; int32_t* compact; uint32_t* active_idx; const double* pixacc;
    double* A22b2; double* pack_head; long head_len; double alpha; const double* Gx; const double* Gy; uint8_t* active_bits; long max_P; long n_ablk;
    // Fused step (blk_cnt != nullptr): no scan launch in between.  Every block sums the counts of the blocks in front of it itself (at most a
    // few thousand L2-resident words), and the LAST block publishes what the host polls for: P, the inlier total (sum of the flag-count
    // blocks of launch A), the status word, then the two sequence words.
    const uint32_t* blk_cnt; const uint32_t* fblk_cnt; long n_fblk; uint32_t* total_P; int* total_P_host; uint32_t* total_inl; int* total_inl_host;
    const int* err_dev; int* err_host; int seq; int* seq_host;
    int bits_head_done;   // launch A has already written the activity bits and cleared the head of the pack
    const uint16_t* seg;  // active_gather_block: launch A's per-unit active lists
    int ablate;           // diagnostics builds only: 2048 no gather / row stores, 4096 no clearing stores, 8192 no lists / active set, 16384 return right after the count loads
    double* clear_pixacc; // non-null (the resident one-GPU step): the per-pixel sums have one reader, this gather — every touched line is zeroed behind it,
                          // so that the next evaluation starts on clean lines without a clearing pass (emba_prep_pose_texel_kernel: no prep blocks)
    const int* blk_rect; int* rect_out;   // non-null: launch A's per-block boxes; the last block reduces them into rect_out = {xmin, ymin, xmax, ymax}
    const int* rect_packed; int* fresh_host;   // with them: the box the texels are packed for; the verdict "the new box lies inside it" (seq, else 0), published in front of the sequence words
};

// the last block's verdict on the packed texels (step_rule.h: rect_contained), in pinned host memory: the host reads it behind the sequence words
__device__ __forceinline__ void publish_texel_verdict(const ActiveWriteParams& a, int xmin, int ymin, int xmax, int ymax)
{
    if (!a.fresh_host) return;
    const bool in = rect_contained(xmin, ymin, xmax, ymax, a.rect_packed[0], a.rect_packed[1], a.rect_packed[2], a.rect_packed[3], kRectFreshSlack);
    a.fresh_host[0] = in ? a.seq : 0;
}

__global__ __launch_bounds__(256) void emba_post_warp_a_kernel(PostWarpParams p)
{
    // A11 = Zero, b1 = Zero (model.cpp:357-361): the head of the pack
    if (p.pack_head) for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.head_len; i += (long)gridDim.x * 256) p.pack_head[i] = 0.0;
    if ((long)blockIdx.x < p.n_ablk) active_count_block(blockIdx.x, p.count, p.npix, p.thres, p.ablk_cnt, p.raw_count, p.pixacc, p.active_bits, p.blk_rect, p.W, p.marker, p.seg, p.clear_inactive, p.global_u8);
    else flag_count_block((long)blockIdx.x - p.n_ablk, p.flag, p.perm, p.n_pm, p.fblk_cnt, p.fsup);
    if (blockIdx.x == 0 && p.fsup_next) for (long i = threadIdx.x; i < p.n_sup; i += 256) p.fsup_next[i * kFlagSupStride] = 0u;    // (two arrays, used alternately: nobody reads or adds to this one during this launch)
}

__device__ __forceinline__ void active_write_block(long blk, const ActiveWriteParams& a)
{   // active_bits: one bit per panorama pixel (pixel p = bit p&31 of 32-bit word p>>5), the Gram kernel's activity lookup
    // compact == nullptr: the pano->compact index map is not needed by this step's consumers (it is produced on demand);
    // alpha != 0: applyL2Reg (model.cpp:689-719) fused into the gather — only legal when no all-reduce follows (single GPU);
    // max_P: rows of A22b2 the (possibly caller-bound) pack has room for — rows past it are not written, the host reports
    // EMBA_ERR_CAPACITY once it has read P.
    // Round 4: the gather is COOPERATIVE.  A lane used to walk its (up to 8) active pixels one after the other — load the line, wait, store the
    // row: as many dependent round trips as the busiest lane of the wave has active pixels, and the zeroing of consumed lines (clear_pixacc)
    // added three scattered stores per touched pixel to the same walk.  Now every wave lists its active pixels by compact rank and its touched
    // pixels in LDS and works through the lists together: 12 pixels x 5 sums per load instruction, two instructions in flight, the rows
    // written as contiguous runs; 10 lines x 6 doubles per clearing store.  The per-block counts in front of the block are fetched in one
    // round trip, issued before the count-map loads.  Same expressions as before: identical values.
    __shared__ uint32_t s_w[4];
    __shared__ uint16_t s_list[4][1024];      // per wave: [0, 512) active pixels by compact rank, [512, 1024) touched pixels
    const int32_t* __restrict__ count = a.count; const double* __restrict__ pixacc = a.pixacc; int32_t* __restrict__ compact = a.compact;
    const long npix = a.npix;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // exclusive prefix of this block over the per-block counts of launch A: up to four independent loads per thread and 1024 blocks
    uint32_t part = 0;
    if (a.blk_cnt) {
        for (long j0 = 0; j0 < blk; j0 += 1024) {
            uint32_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const long j = j0 + threadIdx.x + 256 * u; v[u] = a.blk_cnt[j < a.n_ablk ? j : a.n_ablk - 1]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) if (j0 + threadIdx.x + 256 * u < blk) part += v[u];
        }
    }
    // A11 = Zero, b1 = Zero (model.cpp:357-361): the head of the pack, cleared here so the step needs no memset node
    if (!a.bits_head_done) for (long i = blk * 256 + threadIdx.x; i < a.head_len; i += a.n_ablk * 256) a.pack_head[i] = 0.0;
    const long p0 = blk * kActivePix + 8 * threadIdx.x;
    uint32_t tm = 0;
    const uint32_t m = active_mask8(count, p0, npix, a.thres, &tm);
    if (!a.bits_head_done && p0 < npix) a.active_bits[p0 >> 3] = (uint8_t)m;
    if (EMBA_ABL(a.ablate, 16384) && !(a.blk_cnt && blk == a.n_ablk - 1)) { if (m == 0xFFFFFFFFu) a.active_idx[0] = part; return; }
    const uint32_t mine = __popc(m);
    uint32_t x = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_w[wv] = x;
    uint32_t front = 0;
    if (a.blk_cnt) {
        __shared__ uint32_t s_f[4];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o);
        if (lane == 0) s_f[wv] = part;
        __syncthreads();
        front = (s_f[0] + s_f[1]) + (s_f[2] + s_f[3]);
    } else {
        __syncthreads();
        front = a.blk_off[blk];
    }
    uint32_t wave_base = front;
    for (int w = 0; w < wv; ++w) wave_base += s_w[w];
    uint32_t k = wave_base + x - mine;
    if (a.blk_cnt && blk == a.n_ablk - 1) {   // the last block publishes the step's counts (what launch B did)
        __shared__ uint32_t s_i[4];
        uint32_t parti = 0;
        for (long j = threadIdx.x; j < a.n_fblk; j += 256) parti += a.fblk_cnt[j];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) parti += __shfl_xor(parti, o);
        if (lane == 0) s_i[wv] = parti;
        __syncthreads();
        if (a.blk_rect) {   // the rectangle the NEXT evaluation packs its texels in (and its warp kernel trusts): the box of what this one touched
            __shared__ int s_bx[4][4];
            int xmin = 0x7FFFFFFF, ymin = 0x7FFFFFFF, xmax = -1, ymax = -1;
            for (long j = threadIdx.x; j < a.n_ablk; j += 256) {
                const int4 r = reinterpret_cast<const int4*>(a.blk_rect)[j];
                xmin = min(xmin, r.x); ymin = min(ymin, r.y); xmax = max(xmax, r.z); ymax = max(ymax, r.w);
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                xmin = min(xmin, __shfl_xor(xmin, o)); ymin = min(ymin, __shfl_xor(ymin, o));
                xmax = max(xmax, __shfl_xor(xmax, o)); ymax = max(ymax, __shfl_xor(ymax, o));
            }
            if (lane == 0) { int* bx = s_bx[wv]; bx[0] = xmin; bx[1] = ymin; bx[2] = xmax; bx[3] = ymax; }
            __syncthreads();
            if (threadIdx.x == 0) {
                const int bx0 = min(min(s_bx[0][0], s_bx[1][0]), min(s_bx[2][0], s_bx[3][0])), by0 = min(min(s_bx[0][1], s_bx[1][1]), min(s_bx[2][1], s_bx[3][1]));
                const int bx1 = max(max(s_bx[0][2], s_bx[1][2]), max(s_bx[2][2], s_bx[3][2])), by1 = max(max(s_bx[0][3], s_bx[1][3]), max(s_bx[2][3], s_bx[3][3]));
                a.rect_out[0] = bx0; a.rect_out[1] = by0; a.rect_out[2] = bx1; a.rect_out[3] = by1;
                publish_texel_verdict(a, bx0, by0, bx1, by1);
            }
        }
        if (threadIdx.x == 0) {
            const uint32_t P = front + (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
            const uint32_t n_inl = (s_i[0] + s_i[1]) + (s_i[2] + s_i[3]);
            a.total_P[0] = P; a.total_inl[0] = n_inl;
            if (a.total_P_host) a.total_P_host[0] = (int)P;
            if (a.total_inl_host) a.total_inl_host[0] = (int)n_inl;
            if (a.err_host) a.err_host[0] = a.err_dev[0];
            if (a.seq_host) {
                __threadfence_system();
                __hip_atomic_store(a.seq_host + 0, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(a.seq_host + 1, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
    if (compact && p0 + 8 <= npix) {   // compact index of 8 consecutive pixels: two 16-B stores
        int cv[8];
        uint32_t kk = k;
#pragma unroll
        for (int j = 0; j < 8; ++j) cv[j] = (m & (1u << j)) ? (int)(kk++) : -1;
        reinterpret_cast<int4*>(compact + p0)[0] = make_int4(cv[0], cv[1], cv[2], cv[3]);
        reinterpret_cast<int4*>(compact + p0)[1] = make_int4(cv[4], cv[5], cv[6], cv[7]);
    }
    // the active set, and the wave's lists
    uint16_t* const list = s_list[wv];
    if (!EMBA_ABL(a.ablate, 8192)) {
        uint32_t kk = x - mine;                                               // rank inside the wave
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long i = p0 + j;
            if (m & (1u << j)) {
                if (compact && p0 + 8 > npix) compact[i] = (int32_t)(wave_base + kk);
                a.active_idx[wave_base + kk] = (uint32_t)i;
                list[kk] = (uint16_t)(lane * 8 + j);
                ++kk;
            } else if (compact && p0 + 8 > npix && i < npix) {
                compact[i] = -1;
            }
        }
    }
    const int n_act = __shfl((int)x, 63);
    int n_t = 0;
    if (a.clear_pixacc) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {   // touched pixels (any order)
            const bool t = (tm >> j) & 1u;
            const unsigned long long mk = __ballot(t);
            if (t) list[512 + n_t + (int)__popcll(mk & ((1ull << lane) - 1ull))] = (uint16_t)(lane * 8 + j);
            n_t += (int)__popcll(mk);
        }
    }
    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           // one wave: LDS operations complete in order
    const long wave_p0 = blk * kActivePix + 512L * wv;
    if (a.A22b2 && n_act > 0 && !EMBA_ABL(a.ablate, 2048)) {   // quadratic cost: the per-pixel sums of the warp kernel ARE A22/b2 of the active pixels
        const double alpha = a.alpha;
        const int e5 = lane / 5, comp = lane - 5 * e5;
        for (int g = 0; g < n_act; g += 24) {                         // two instructions of 12 pixels x 5 sums in flight
            const int ea = g + e5, eb = g + 12 + e5;
            const bool oka = lane < 60 && ea < n_act, okb = lane < 60 && eb < n_act;
            const long pa = wave_p0 + list[oka ? ea : 0], pb = wave_p0 + list[okb ? eb : 0];
            // (unconditional loads — a lane without an entry re-reads the wave's first active pixel: a load under a lane mask is waited for
            // at the end of its branch, and the two instructions would run one after the other)
            double va = pixacc[(size_t)kPixAccStride * pa + comp], vb = pixacc[(size_t)kPixAccStride * pb + comp];
            if (alpha != 0.0) {                                       // (wave-uniform) applyL2Reg, model.cpp:689-719
                const double* G = (comp == 4) ? a.Gy : a.Gx;
                const double ga = G[pa], gb = G[pb];
                if (comp == 0 || comp == 2) { va = va + alpha; vb = vb + alpha; }
                else if (comp >= 3) { va = va - alpha * ga; vb = vb - alpha * gb; }
            }
            if (oka && (long)(wave_base + ea) < a.max_P) a.A22b2[5 * (size_t)(wave_base + ea) + comp] = va;
            if (okb && (long)(wave_base + eb) < a.max_P) a.A22b2[5 * (size_t)(wave_base + eb) + comp] = vb;
        }
    }
    if (a.clear_pixacc && n_t > 0 && !EMBA_ABL(a.ablate, 4096)) {
        __builtin_amdgcn_s_waitcnt(0x0F70);                           // vmcnt(0): the gathers above have returned before their lines are zeroed
        const int e6 = lane / 6, comp = lane - 6 * e6;
        for (int g = 0; g < n_t; g += 10) {
            const int e = g + e6;
            if (lane < 60 && e < n_t) a.clear_pixacc[(size_t)kPixAccStride * (wave_p0 + list[512 + e]) + comp] = 0.0;
        }
    }
}

__global__ __launch_bounds__(256) void emba_active_write_kernel(ActiveWriteParams a) { active_write_block(blockIdx.x, a); }

// ------------------------------------------------------------------------------------------------
// a8 + the A22 | b2 gather of the resident one-GPU step, LIST-DRIVEN.  Round 4, measured (scripts/r04_exp5.sh): of the 15 us of the
// sweeping write kernel above, 7.7 are its launch + one pass over the 8-MB count map, and 5.8 the gather — the active pixels sit in the
// ~8 % of the panorama the camera looked at, so a few dozen of the 1024 blocks do all of it, one dependent round trip per 24 pixels of a
// wave that has hundreds.  Launch A (active_count_block) now leaves every unit's active pixels as a list; here a block takes an EQUAL slice
// [k0, k1) of the compact index range: prefix of the per-unit counts in LDS, binary search k -> (unit, rank), list entry -> pixel, then 8
// lanes fetch one pixel's 64-B accumulator line (all of a slice's lines in flight at once), write its row of the pack (applyL2Reg folded in,
// model.cpp:689-719) and the active-set entry, and zero the line behind the gather.  Work proportional to P, balanced, no count-map pass.
// Used as the head of the Gram kernel (gram_body<.., GATHER>: no launch of its own) or as a kernel of its own.  s_pre: kGatherMaxUnits + 1 words,
// s_ws: NT / 64.  (Round 4 also tried a "compact" Gram kernel under it — a wave lists its chunk's live slots first and then fetches only those,
// every lane of every load useful, half the stages: 27.3 vs 27.8 us at 1 M events, 62.6 vs 45.6 us at 1.5 M: the stream form's time is the
// records' 7 TB/s burst plus fixed costs, not its chain of stages — s_memtime stamps per wave: phase A 2.6 us, records 9.1, wave flush 3.2,
// final barrier 2.8 of a 17.8-us wave in a 27-us kernel.  Dropped.)
// ------------------------------------------------------------------------------------------------
constexpr int kGatherMaxUnits = 4096;    // panoramas up to 8 M pixels (2048 x 4096); beyond that the host keeps the sweeping form
// part 1: the prefix of the per-unit counts in s_pre (two barriers), what block 0 publishes; returns P.
template <int NT>
__device__ __forceinline__ uint32_t active_gather_prefix(const ActiveWriteParams& a, long blk, uint32_t* s_pre, uint32_t* s_ws)
{
    constexpr int NW = NT / 64, PER = (kGatherMaxUnits + NT - 1) / NT;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __shared__ int s_pub[NW][5];
    if (blk == 0) {   // (block-uniform) block 0 also publishes what the host polls for: the inlier total and the next evaluation's texel rectangle ride
                      // through the same two barriers as the prefix below — every thread fetches its share at once (a single wave walking the
                      // per-block arrays, one dependent load after the other, held this block back by ~8 us)
        uint32_t ni = 0;
        for (long j = tid; j < a.n_fblk; j += NT) ni += a.fblk_cnt[j];
        int xmin = 0x7FFFFFFF, ymin = 0x7FFFFFFF, xmax = -1, ymax = -1;
        if (a.blk_rect)
            for (long j = tid; j < a.n_ablk; j += NT) {
                const int4 r = reinterpret_cast<const int4*>(a.blk_rect)[j];
                xmin = min(xmin, r.x); ymin = min(ymin, r.y); xmax = max(xmax, r.z); ymax = max(ymax, r.w);
            }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            ni += __shfl_xor(ni, o);
            xmin = min(xmin, __shfl_xor(xmin, o)); ymin = min(ymin, __shfl_xor(ymin, o));
            xmax = max(xmax, __shfl_xor(xmax, o)); ymax = max(ymax, __shfl_xor(ymax, o));
        }
        if (lane == 0) { s_pub[wv][0] = (int)ni; s_pub[wv][1] = xmin; s_pub[wv][2] = ymin; s_pub[wv][3] = xmax; s_pub[wv][4] = ymax; }
    }
    // exclusive prefix of launch A's per-unit counts -> s_pre[0 .. n_ablk], s_pre[n_ablk] = P
    uint32_t v[PER], mine = 0;
#pragma unroll
    for (int u = 0; u < PER; ++u) { const long j = (long)tid * PER + u; v[u] = a.blk_cnt[j < a.n_ablk ? j : a.n_ablk - 1]; }
#pragma unroll
    for (int u = 0; u < PER; ++u) { if ((long)tid * PER + u >= a.n_ablk) v[u] = 0; mine += v[u]; }
    uint32_t x = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o); if (lane >= o) x += y; }
    if (lane == 63) s_ws[wv] = x;
    __syncthreads();
    uint32_t woff = 0, P = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { const uint32_t t = s_ws[w]; P += t; if (w < wv) woff += t; }
    {
        uint32_t run = woff + x - mine;
#pragma unroll
        for (int u = 0; u < PER; ++u) { const long j = (long)tid * PER + u; if (j < a.n_ablk) s_pre[j] = run; run += v[u]; }
        if (tid == 0) s_pre[a.n_ablk] = P;
    }
    if (blk == 0 && tid == 0) {
        uint32_t ni = 0; int xmin = 0x7FFFFFFF, ymin = 0x7FFFFFFF, xmax = -1, ymax = -1;
        for (int w = 0; w < NW; ++w) { ni += (uint32_t)s_pub[w][0]; xmin = min(xmin, s_pub[w][1]); ymin = min(ymin, s_pub[w][2]); xmax = max(xmax, s_pub[w][3]); ymax = max(ymax, s_pub[w][4]); }
        if (a.blk_rect) { a.rect_out[0] = xmin; a.rect_out[1] = ymin; a.rect_out[2] = xmax; a.rect_out[3] = ymax; publish_texel_verdict(a, xmin, ymin, xmax, ymax); }
        a.total_P[0] = P; a.total_inl[0] = ni;
        if (a.total_P_host) a.total_P_host[0] = (int)P;
        if (a.total_inl_host) a.total_inl_host[0] = (int)ni;
        if (a.err_host) a.err_host[0] = a.err_dev[0];
        if (a.seq_host) {
            __threadfence_system();
            __hip_atomic_store(a.seq_host + 0, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(a.seq_host + 1, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    __syncthreads();
    return P;
}

// part 2: the block's slice of the compact index range (see above)
template <int NT>
__device__ __forceinline__ void active_gather_slice(const ActiveWriteParams& a, long blk, long nblk, uint32_t P, const uint32_t* s_pre)
{
    constexpr int Q = GATHER_Q, PIX = NT / 8;   // PIX pixels per pass of the block (8 lanes each), Q passes in flight
    const int tid = threadIdx.x;
    const long per = ((long)P + nblk - 1) / nblk;
    const long k0 = blk * per, k1 = (k0 + per < (long)P) ? k0 + per : (long)P;
    const int comp = tid & 7;
    const double alpha = a.alpha;
    const int n_units = (int)a.n_ablk;
    for (long base = k0; base < k1; base += (long)Q * PIX) {       // block-uniform; one trip at the BASELINE workload (P / grid = 270 pixels)
        long kq[Q]; bool ok[Q]; int lo[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) { const long k = base + (long)q * PIX + (tid >> 3); ok[q] = k < k1; kq[q] = ok[q] ? k : k0; lo[q] = 0; }
        // the unit of k: the LAST u with s_pre[u] <= k (units in front of it may be empty) — a fixed-length, branch-free search, the Q of them
        // side by side (a data-dependent loop per pass runs its dozen LDS round trips one pass after the other)
#pragma unroll
        for (int step = kGatherMaxUnits / 2; step >= 1; step >>= 1)
#pragma unroll
            for (int q = 0; q < Q; ++q) { const int cand = lo[q] + step; if (cand < n_units && (long)s_pre[cand < n_units ? cand : 0] <= kq[q]) lo[q] = cand; }
        long pix[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) pix[q] = (long)lo[q] * kActivePix + a.seg[(size_t)lo[q] * kActivePix + (kq[q] - (long)s_pre[lo[q]])];
        double val[Q], g[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) val[q] = a.pixacc[(size_t)kPixAccStride * pix[q] + comp];   // 8 lanes = one 64-B line; every pass in flight
        if (alpha != 0.0) {
            const double* G = (comp == 4) ? a.Gy : a.Gx;
#pragma unroll
            for (int q = 0; q < Q; ++q) g[q] = G[pix[q]];
        }
        if (a.clear_pixacc) {   // the lines are zeroed behind the gather — FIRST, while only the loads above are outstanding (the wait does not include a store)
            __builtin_amdgcn_s_waitcnt(0x0F70);                       // vmcnt(0): every lane of every pass has its value
#pragma unroll
            for (int q = 0; q < Q; ++q) if (ok[q] && comp < 6) a.clear_pixacc[(size_t)kPixAccStride * pix[q] + comp] = 0.0;
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            double w = val[q];
            if (alpha != 0.0) {
                if (comp == 0 || comp == 2) w = w + alpha;
                else if (comp == 3 || comp == 4) w = w - alpha * g[q];
            }
            if (ok[q] && !EMBA_ABL(a.ablate, 2048)) {
                if (comp < 5 && kq[q] < a.max_P) a.A22b2[5 * (size_t)kq[q] + comp] = w;
                if (comp == 5) a.active_idx[kq[q]] = (uint32_t)pix[q];
            }
        }
    }
}

__global__ __launch_bounds__(256) void emba_active_gather_kernel(ActiveWriteParams a)
{
    __shared__ uint32_t s_pre[kGatherMaxUnits + 1];
    __shared__ uint32_t s_ws[4];
    const uint32_t P = active_gather_prefix<256>(a, blockIdx.x, s_pre, s_ws);
    active_gather_slice<256>(a, blockIdx.x, gridDim.x, P, s_pre);
}



// Exchange-1 compression straight from the warp kernel's markers (round 5): the rank's counts are materialised (markers -> the count in the sixth double of the
// pixel's accumulator line; whatever an earlier evaluation left -> 0) and their saturated bytes written in the same pass — one sweep of the map instead of two.
__global__ __launch_bounds__(256) void emba_count_materialise_compress_kernel(int32_t* __restrict__ count, const double* __restrict__ pixacc, long npix, int32_t marker,
                                                                              int cap, uint8_t* __restrict__ out)
{
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (p0 >= npix) return;
    int c[8];
    (void)materialise_mask8(count, pixacc, p0, npix, 1, marker, nullptr, c);
    if (p0 + 8 <= npix) {
        uint2 o;
        o.x = (uint32_t)min(c[0], cap) | ((uint32_t)min(c[1], cap) << 8) | ((uint32_t)min(c[2], cap) << 16) | ((uint32_t)min(c[3], cap) << 24);
        o.y = (uint32_t)min(c[4], cap) | ((uint32_t)min(c[5], cap) << 8) | ((uint32_t)min(c[6], cap) << 16) | ((uint32_t)min(c[7], cap) << 24);
        *reinterpret_cast<uint2*>(out + p0) = o;
    } else {
        for (int k = 0; k < 8; ++k) if (p0 + k < npix) out[p0 + k] = (uint8_t)min(c[k], cap);
    }
}

// Exchange-1 compression: int32 counts <-> saturated bytes (4 pixels per thread)
__global__ void emba_count_compress_kernel(const int32_t* __restrict__ count, long npix, int cap, uint8_t* __restrict__ out)
{
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (p0 + 4 <= npix) {
        const int4 c = *reinterpret_cast<const int4*>(count + p0);
        uchar4 o;
        o.x = (unsigned char)min(c.x, cap); o.y = (unsigned char)min(c.y, cap); o.z = (unsigned char)min(c.z, cap); o.w = (unsigned char)min(c.w, cap);
        *reinterpret_cast<uchar4*>(out + p0) = o;
    } else {
        for (long i = p0; i < npix; ++i) out[i] = (uint8_t)min(count[i], cap);
    }
}

__global__ void emba_count_expand_kernel(const uint8_t* __restrict__ in, long npix, int32_t* __restrict__ count)
{
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (p0 + 4 <= npix) {
        const uchar4 c = *reinterpret_cast<const uchar4*>(in + p0);
        *reinterpret_cast<int4*>(count + p0) = make_int4(c.x, c.y, c.z, c.w);
    } else {
        for (long i = p0; i < npix; ++i) count[i] = in[i];
    }
}

// pano -> compact index map from the active list (on demand: generic A22 path, dense/sparse A12 export, Schur solve)
__global__ void emba_compact_map_kernel(const uint32_t* __restrict__ active_idx, const uint32_t* __restrict__ P_dev, int32_t* __restrict__ compact)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (long)P_dev[0]) compact[active_idx[i]] = (int32_t)i;
}

// Start of an evaluation ("prep"): zero the count map (model.cpp:85) and the pixacc lines the previous evaluation touched
// (`count` still holds the previous, possibly all-reduced, counts: a superset of the locally touched pixels).
__device__ __forceinline__ void prep_block(long blk, int32_t* __restrict__ count, long npix, double* __restrict__ pixacc)
{
    const long p0 = (blk * 256 + threadIdx.x) * 4;
    if (p0 >= npix) return;
    int cc[4] = {0, 0, 0, 0};
    if (p0 + 4 <= npix) {
        const int4 c = *reinterpret_cast<const int4*>(count + p0);
        cc[0] = c.x; cc[1] = c.y; cc[2] = c.z; cc[3] = c.w;
        if ((c.x | c.y | c.z | c.w) != 0) *reinterpret_cast<int4*>(count + p0) = make_int4(0, 0, 0, 0);
    } else {
        for (int k = 0; k < 4 && p0 + k < npix; ++k) { cc[k] = count[p0 + k]; if (cc[k]) count[p0 + k] = 0; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (cc[k] != 0) {
            double2* a = reinterpret_cast<double2*>(pixacc + (size_t)kPixAccStride * (p0 + k));
            a[0] = make_double2(0, 0); a[1] = make_double2(0, 0); a[2] = make_double2(0, 0);
        }
}

// ONE launch in front of the warp kernel (was two: prep, then pose || texel): the three jobs are independent of each other —
//   n_pose blocks   a2/a3 pose table (pixel order) or the K-1 segment records (tile order)
//   n_tex blocks    texel pack inside the rectangle of the pixels the last FORMED evaluation touched (reduced by its post-warp kernels; a hint
//                   only: outside it the warp kernel falls back to the stencil)
//   n_prep blocks   "prep": zero the count map (model.cpp:85) and the pixacc lines the previous evaluation touched (`count` still holds the
//                   previous, possibly all-reduced, counts or that evaluation's markers: a superset of the locally touched pixels).  NONE when
//                   the previous evaluation's sums were consumed and cleared by the resident step's gather (ActiveWriteParams::clear_pixacc):
//                   the count map itself never needs clearing — its entries are stamped (count_marker)
// The control poses travel BY VALUE in the kernel arguments (K <= kInlineKnots: no staging copy, no dependency on another block);
// larger K reads them from `knots_dev`, which the host has copied there before the launch.
// err_next: the status word of the NEXT evaluation, cleared here (this launch's pose threads may already be setting bits of err).
struct PrepPoseTexelParams {
    int32_t* count; long npix; double* pixacc; int W, H; int n_prep;
    const int64_t* batch_t_ns; int nb; int K; int64_t t0_ns, dt_ns; double* pose; int* err; int* err_next; int n_pose; double* seg;
    const double* knots_dev; double* knots_out; int inline_knots;
    int n_tex; const double* Gx; const double* Gy; const int* rect; double* texel;
    int* rect_packed;   // n_tex != 0: the box the texels are packed for from now on (= rect), what the warp kernel trusts
};

__global__ __launch_bounds__(256) void emba_prep_pose_texel_kernel(PrepPoseTexelParams p, InlineKnots kn)
{
    // block order = start order: the pose threads first (one long dependent chain each: the launch's critical path), then the texel
    // blocks, the prep blocks (many, short) fill in behind
    const int b = (int)blockIdx.x;
    if (b == 0) {   // (whatever block 0's role is; none of the roles below has a barrier)
        if (threadIdx.x == 255) p.err_next[0] = 0;
        if (p.n_tex && threadIdx.x >= 248 && threadIdx.x < 252) p.rect_packed[threadIdx.x - 248] = p.rect[threadIdx.x - 248];   // (the texel blocks read rect, the warp kernel rect_packed)
        if (p.inline_knots && p.knots_out) for (int i = (int)threadIdx.x - 64; i >= 0 && i < 4 * p.K; i += 192) p.knots_out[i] = kn.q[i];   // (for whoever reads the device copy later)
    }
    if (b < p.n_pose) {
        if (threadIdx.x < 64) {
            const double* knots = p.inline_knots ? kn.q : p.knots_dev;
            const int i = b * 64 + threadIdx.x;
            if (p.seg) seg_thread(i, knots, p.K, p.seg);
            else pose_thread(i, p.batch_t_ns, p.nb, knots, p.K, p.t0_ns, p.dt_ns, p.pose, p.err);
        }
    } else if (b < p.n_pose + p.n_tex) {
        texel_rect_blocks((long)b - p.n_pose, p.n_tex, p.Gx, p.Gy, p.H, p.W, p.rect, p.texel);
    } else {
        prep_block(b - p.n_pose - p.n_tex, p.count, p.npix, p.pixacc);
    }
}

// ------------------------------------------------------------------------------------------------
// a9/a10: A11 / b1 as a batched Gram-matrix contraction on the fp64 matrix cores.
// The 128-B factor record IS a 16-vector r = [jc(6) jp(6) dp(2) e tail]; for records that share the control-pose pair
// (cp_c, cp_p), sum_k w_k r_k r_k^T holds every block the reference accumulates (model.cpp:454-477):
//     rows/cols 0-5 x 0-5  -> A11(c,c)    0-5 x 6-11 -> A11(c,p)    6-11 x 0-5 -> A11(p,c)    6-11 x 6-11 -> A11(p,p)
//     rows 0-11 of column 14 (e)           -> b1(c), b1(p)           (rows/cols 12-15 are by-products and are dropped)
// v_mfma_f64_16x16x4_f64 consumes 4 records per instruction straight from a fully coalesced 512-B load (lane l holds
// element l&15 of record l>>4, exactly the A/B operand layout), the accumulator is 4 doubles per lane, and the flush
// needs no cross-lane reduction: lane l owns D[(l>>4)+4r][l&15].  Records are sorted by pair, so a wave flushes (fp64
// atomics, <= 4 per lane) only when the pair changes or its chunk ends.  IRLS weights (model.cpp:599-618) scale the A operand.
// ------------------------------------------------------------------------------------------------
typedef double double4_t __attribute__((ext_vector_type(4)));

struct GramParams {
    const double* rec; const uint32_t* slot_key; long n_slots; int chunk;   // chunk: record slots per wave (multiple of 8)
    const uint32_t* active_bits; int irls; double eta;                    // active_bits: count >= thres per pixel (model.cpp:333,409)
    uint32_t stamp;                                                       // records of the current evaluation (record_valid)
    const double* tag;                                                    // per slot {pano pixel, stamp} (8 B), or nullptr: decide from the records themselves
    double* A11; double* b1; int dim;  // dim = 3K
    int ablate;  // diagnostics only: 32 no flush atomics, 64 no MFMA
    int gather_waves;  // GATHER form: 1, 2 or 4 of the block's 16 waves do its slice of the active-set gather, the others stream (host: by size)
    int n_gram_blocks; // blocks [0, n_gram_blocks) of the grid form the Gram sums; the blocks behind them (the resident step, ep_out != nullptr) compact the
                       // residuals into the reference-order ep vector (ep_tail_block): no launch and no scan launch of their own
    const uint8_t* ep_flag; const double* ep_e; double* ep_out; const uint32_t* ep_fblk_cnt; long ep_n_pm, ep_n_fblk; const uint32_t* ep_fsup;
    const uint32_t* wave_cuts;   // PAIRED form: [start, end) per wave slot (kGramBlock / 64 per block), each inside one pair's run of slots (step_rule.h: gram_pair_cuts)
};

// Global flush of one 16x16 tile value owned by (row, col) for the pair `key`.
__device__ __forceinline__ void gram_atomic_out(double v, int row, int col, uint32_t key, double* A11, double* b1, int dim, int ablate)
{
    if (row >= 12 || v == 0.0 || EMBA_ABL(ablate, 32)) return;
    const int bc = 3 * (int)(key >> 16), bp = 3 * (int)(key & 0xFFFFu);
    const int grow = (row < 6) ? bc + row : bp + row - 6;
    if (col < 12) {
        const int gcol = (col < 6) ? bc + col : bp + col - 6;
        atomicAdd(A11 + (size_t)grow + (size_t)dim * gcol, v);
    } else if (col == 14) {
        atomicAdd(b1 + grow, v);
    }
}

// Operand layout of the Gram kernel.  A wave-instruction loads 8 consecutive records as 16 B per lane (1 KiB, the access width
// HBM streams fastest at): lane l holds elements (2m, 2m+1), m = l&7, of record R = l>>3.  Fed to v_mfma_f64_16x16x4_f64 as they
// stand (operand row/col index l&15 = 8(R&1)+m, k index l>>4 = R>>1), the products of the EVEN elements give
//     D[i][j] = sum_k r_{2k}[2i] r_{2k}[2j]  (i,j < 8: even records)   and   D[8+i][8+j] = the same over the odd records,
// the two off-diagonal quadrants mix records and are ignored.  Three MFMAs (even x even, odd x even, odd x odd elements) per 8
// records therefore hold the whole symmetric 16x16 Gram sum, with no cross-lane data movement at all.
//
// A wave hands its three tiles to the block's LDS combine table (fp64 LDS atomics; one 16x16 table per pair, kGramKeys pairs
// per block) so that the 16 waves of a block cost ONE set of global atomics per pair instead of 16 — the global fp64 atomics
// all land on the few A11 blocks of the current pairs and serialise at the memory side otherwise.  Called once or twice per
// wave: a real function (arguments by value, in registers), so that its index arithmetic stays out of the streaming loop.
// (a real call: 31 argument registers — the two LDS tables travel as 16-bit LDS addresses in one word and dim | ablate in another, or the last arguments would go
// through the stack: 16 B of scratch per lane in every Gram kernel until round 6)
typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
typedef __attribute__((address_space(3))) double lds_f64_t;
__device__ __attribute__((noinline)) void gram_flush(double4_t ee, double4_t oe, double4_t oo, uint32_t key, double* A11, double* b1,
                                                     uint32_t dim_ablate, uint32_t lds_tag_tile)
{
    const int dim = (int)(dim_ablate & 0x3FFFFu), ablate = (int)(dim_ablate >> 18);      // (dim = 3K <= 196 605; the diagnostics mask fits 14 bits)
    uint32_t* const s_tag = (uint32_t*)(lds_u32_t*)(uintptr_t)((lds_tag_tile & 0xFFFFu) << 2);      // (LDS addresses in units of the tables' element sizes: 160 KB fit)
    double* const s_tile = (double*)(lds_f64_t*)(uintptr_t)((lds_tag_tile >> 16) << 3);
    const int lane = threadIdx.x & 63;
    int slot = -1;
    if (lane == 0) {
        for (int k = 0; k < kGramKeys; ++k) {
            const uint32_t old = atomicCAS(&s_tag[k], 0xFFFFFFFFu, key);
            if (old == 0xFFFFFFFFu || old == key) { slot = k; break; }
        }
    }
    slot = __shfl(slot, 0);
    auto out = [&](double v, int row, int col) {   // entry (row, col) of the symmetric 16x16 sum; rows >= 12 and cols 12, 13, 15 are not used
        if (v == 0.0 || row >= 12 || !(col < 12 || col == 14)) return;
        if (slot >= 0) atomicAdd(&s_tile[slot * 256 + row * 16 + col], v);
        else gram_atomic_out(v, row, col, key, A11, b1, dim, ablate);
    };
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = (lane >> 4) + 4 * r, j = lane & 15;      // C/D layout of v_mfma_f64_16x16x4_f64
        if ((i >> 3) == (j >> 3)) {                             // same-record quadrants only
            const int i2 = 2 * (i & 7), j2 = 2 * (j & 7);
            out(ee[r], i2, j2);
            out(oe[r], i2 + 1, j2);
            out(oe[r], j2, i2 + 1);                             // even x odd = transpose of odd x even
            out(oo[r], i2 + 1, j2 + 1);
        }
    }
}

// The wave's LAST flush (round 5): its symmetric 16 x 16 sum as 256 plain LDS stores into the wave's own tile instead of ~16 fp64 LDS atomics per lane into the
// block's shared table, where the sixteen waves of a block queued on the same 156 addresses (s_memtime stamps, round 4: 3.2 us per wave in the flush and 2.8 in the
// barrier behind it, of a 17.8-us wave).  The two same-record quadrants of an accumulator (lanes j < 8 with rows i < 8: the even records; lanes j >= 8 with rows
// i >= 8: the odd ones) are first added by a DPP row shift — lane (q, j) takes lane (q, j + 8) — then the 32 lanes j < 8 store ee -> (2i, 2j), oe -> (2i+1, 2j) and
// its transpose, oo -> (2i+1, 2j+1): every entry of the tile exactly once.  The block sums the waves' tiles per control-pose pair after its final barrier.
__device__ __forceinline__ double dpp_row_shl8(double v)      // lane l <- lane l + 8 of its row of 16 (0 where there is none)
{
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x108, 0xf, 0xf, true),
                            __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x108, 0xf, 0xf, true));
}
__device__ __forceinline__ void gram_wave_tile(double4_t ee, double4_t oe, double4_t oo, double* __restrict__ tile)
{
    const int lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const double e = ee[r] + dpp_row_shl8(ee[r + 2]), x = oe[r] + dpp_row_shl8(oe[r + 2]), o = oo[r] + dpp_row_shl8(oo[r + 2]);
        if (j < 8) {
            const int i = q + 4 * r;
            tile[(2 * i) * 16 + 2 * j] = e;
            tile[(2 * i + 1) * 16 + 2 * j] = x;
            tile[(2 * j) * 16 + 2 * i + 1] = x;
            tile[(2 * i + 1) * 16 + 2 * j + 1] = o;
        }
    }
}

// elements 14 (residual) and 15 ({pano_idx, aux}) of the record whose 8 lanes this lane belongs to: they sit in lane 8R+7
// (ds_swizzle bit-mask mode inside 32 lanes: lane' = (lane & 0x18) | 7; no address VGPR, no memory request)
__device__ __forceinline__ double rec_elem14(double2 v)
{
    return __hiloint2double(__builtin_amdgcn_ds_swizzle(__double2hiint(v.x), (7 << 5) | 0x18),
                            __builtin_amdgcn_ds_swizzle(__double2loint(v.x), (7 << 5) | 0x18));
}
__device__ __forceinline__ uint32_t rec_elem15_lo(double2 v)
{
    return (uint32_t)__builtin_amdgcn_ds_swizzle(__double2loint(v.y), (7 << 5) | 0x18);
}
__device__ __forceinline__ uint32_t rec_elem15_hi(double2 v)
{
    return (uint32_t)__builtin_amdgcn_ds_swizzle(__double2hiint(v.y), (7 << 5) | 0x18);
}

// GATHER (the resident one-GPU step): every block first does its slice of the list-driven active-set write + A22 | b2 gather (active_gather_*): it
// only depends on launch A of the post-warp pair, like the Gram sums, and as a prologue it costs three short round trips instead of a launch of
// its own with a pass over the count map (round 4, 1 M events: 27.5 + 15 us -> 34.5 us).
// PAIRED (with TAGS, dense): every streaming wave has a slot range of its own inside ONE pair's run (p.wave_cuts) instead of a share of the block's window: no pair
// change in mid-stream, so no flush but the wave's tile at its end, no key table, no LDS atomics; the block sums the tiles per pair in wave order.
template <bool TAGS, int kGramBlock, bool GATHER, bool SPARSE = false, bool PAIRED = false>   // TAGS: p.tag is the per-slot tag stream (pixel order); otherwise activity is decided from the records (tile order).  SPARSE (with TAGS): few slots live — stages of 128 tags, compacted
__device__ __forceinline__ void gram_body(const GramParams& p, const long gram_blk, const ActiveWriteParams& aw)
{
    __shared__ uint32_t s_tag[kGramKeys];
    __shared__ double s_tile[kGramKeys * 256];
    __shared__ uint32_t s_pre[GATHER ? kGatherMaxUnits + 1 : 1];
    __shared__ uint32_t s_ws[kGramBlock / 64];
    __shared__ double s_wtile[(kGramBlock / 64) * 256];      // every wave's own 16 x 16 sum of its last pair (gram_wave_tile)
    __shared__ uint32_t s_wkey[kGramBlock / 64];
    static_assert(!PAIRED || (TAGS && !SPARSE && GRAM_WAVE_TILE), "the pair-aligned form is the dense tag-stream form with the waves' own tiles");
    if constexpr (!PAIRED) {
        for (int i = threadIdx.x; i < kGramKeys * 256; i += kGramBlock) s_tile[i] = 0.0;
        if (threadIdx.x < kGramKeys) s_tag[threadIdx.x] = 0xFFFFFFFFu;
    }
    if (threadIdx.x < kGramBlock / 64) s_wkey[threadIdx.x] = 0xFFFFFFFFu;
    // GATHER: the block's slice of the gather is the work of its first kGW waves ONLY; the others go straight to the record stream, which depends on
    // launch A's activity bits and on nothing the gather writes (round 4, late: with all 16 waves gathering first the head cost this kernel 9 us
    // of dependent round trips in front of its stream; now they run beside it)
    // How many: p.gather_waves (the host passes 4; 1 and 2 were measured, scripts/r04_exp15.sh: one wave's gather outlasts the stream at every size).
    const int kGW = GATHER ? __builtin_amdgcn_readfirstlane(p.gather_waves) : 0, kSW = kGramBlock / 64 - kGW;
    if (GATHER) {   // (its two barriers also publish the cleared combine table)
        const uint32_t P_act = active_gather_prefix<kGramBlock>(aw, gram_blk, s_pre, s_ws);
        if (threadIdx.x < 64 * kGW) {
            if (kGW == 1) active_gather_slice<64>(aw, gram_blk, p.n_gram_blocks, P_act, s_pre);
            else if (kGW == 2) active_gather_slice<128>(aw, gram_blk, p.n_gram_blocks, P_act, s_pre);
            else active_gather_slice<256>(aw, gram_blk, p.n_gram_blocks, P_act, s_pre);
        }
    } else {
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) - kGW;      // index among the streaming waves (< 0: a gather wave)
    // The block's 16 waves walk ONE contiguous range of 16 x chunk record slots together, stage by stage (wave w takes stages
    // w, w+16, ...): at any moment the block reads a compact window of the stream, as a grid-stride loop would, instead of 16
    // separate streams 128 KB apart (4096 concurrent streams chip-wide cost DRAM page locality once the records exceed the
    // Infinity Cache).  Which wave sums which record is immaterial: everything of a pair meets in the block's LDS table.
    constexpr int U = TAGS ? GRAM_U : GRAM_U_NT;   // independent 1-KiB loads (8 records each) per wave and stage
    constexpr int TS = GRAM_SPARSE_TS;             // SPARSE: tag loads (64 slots each) per wave and stage
    constexpr int kStage = SPARSE ? 64 * TS : 8 * U;
    const int kStride = PAIRED ? kStage : kSW * kStage;
    long start, end;
    if constexpr (PAIRED) {      // the wave's own range (a gather wave reads slot 0's and does not use it)
        const uint32_t* cut = p.wave_cuts + 2 * (gram_blk * (kGramBlock / 64) + (wv > 0 ? wv : 0));
        start = (long)__builtin_amdgcn_readfirstlane((int)cut[0]);
        end = (long)__builtin_amdgcn_readfirstlane((int)cut[1]);
    } else {
        start = gram_blk * (kGramBlock / 64) * p.chunk;
        end = (start + (long)(kGramBlock / 64) * p.chunk < p.n_slots) ? start + (long)(kGramBlock / 64) * p.chunk : p.n_slots;
    }
    const int len = (int)(end - start);                              // <= 16 * kGramChunk: stage offsets are 32-bit
    const int off0 = PAIRED ? 0 : wv * kStage;
    const bool have_work = wv >= 0 && off0 < len;   // wave-uniform
    const int m = lane & 7, R = lane >> 3;
    if (have_work) {

    uint32_t cur_key = p.slot_key[start + off0];
    bool dirty = false;
    double4_t acc_ee = {0.0, 0.0, 0.0, 0.0}, acc_oe = acc_ee, acc_oo = acc_ee;
    auto flush = [&]() {
        gram_flush(acc_ee, acc_oe, acc_oo, cur_key, p.A11, p.b1, (uint32_t)p.dim | ((uint32_t)p.ablate << 18),
                   (((uint32_t)(uintptr_t)(lds_u32_t*)s_tag >> 2) & 0xFFFFu) | (((uint32_t)(uintptr_t)(lds_f64_t*)s_tile >> 3) << 16));
#pragma unroll
        for (int r = 0; r < 4; ++r) { acc_ee[r] = 0.0; acc_oe[r] = 0.0; acc_oo[r] = 0.0; }
    };
    // One fully coalesced 16-B-per-lane load per 8 records is ALL the fast path reads: the residual and the pixel index of a
    // record come from its last lane (ds_swizzle), the pair key is wave-uniform (slots are sorted by pair, so equal first and
    // last keys of a stage mean one pair), and activity comes from a 1-bit map that stays in L2.  Two stages in flight: B's
    // records are on their way while A's activity lookups and MFMAs run.
    double2 xA[U], xB[U];
    uint32_t act[U], k_first = 0, k_last = 0;
    const double2* rec0 = reinterpret_cast<const double2*>(p.rec + (size_t)kRecStride * start) + lane;
    const uint32_t* key0 = p.slot_key + start;
    auto load_records = [&](int off, double2* x) {   // may run up to 8 U records past `end`: the record buffer is padded
        const double2* q = rec0 + 8 * off;           // (kGramPad) and those slots are masked
#pragma unroll
        for (int u = 0; u < U; ++u) {
            typedef double v2d __attribute__((ext_vector_type(2)));
            if (GRAM_NT_LOAD) { const v2d v = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(q + 64 * u)); x[u] = make_double2(v.x, v.y); }
            else x[u] = q[64 * u];
        }
    };
    auto lookup = [&](int off, const double2* x) {
        // first and last pair key of the stage (uniform addresses), issued ahead of the next stage's records
        k_first = key0[off];
        k_last = key0[(off + 8 * U < len ? off + 8 * U : len) - 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t pi = rec_elem15_lo(x[u]);
            const bool in = off + 8 * u + R < len;
            const bool valid = in && rec_elem15_hi(x[u]) == p.stamp && pi != kInvalidPix;
            act[u] = valid ? (EMBA_ABL(p.ablate, 256) ? ~0u : p.active_bits[pi >> 5]) >> (pi & 31) : 0u;
        }
    };
    auto weight = [&](const double2& x) {
        double w = 1.0;
        if (p.irls) {
            const double e = rec_elem14(x);
            if (p.irls == 2) w = 1.0 / (1.0 + p.eta * e * e);          // cauchy, model.cpp:603
            else { const double a = fabs(e); w = (a < p.eta) ? 1.0 : p.eta / a; }   // huber, :608-616
        }
        return w;
    };
    auto consume = [&](int off, double2* x) {
        if (PAIRED || ((k_first == cur_key) && (k_last == cur_key))) {             // fast path: the whole stage belongs to the current pair
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool ok = act[u] & 1u;                               // model.cpp:396,409
                const double w = weight(x[u]);
                // selects, not multiplies: stale slots may hold anything
                const double ax = ok ? w * x[u].x : 0.0, ay = ok ? w * x[u].y : 0.0, bx = ok ? x[u].x : 0.0, by = ok ? x[u].y : 0.0;
                if (__ballot(ok)) {
                    dirty = true;
                    if (!EMBA_ABL(p.ablate, 64)) {
                        acc_ee = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, bx, acc_ee, 0, 0, 0);
                        acc_oe = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, bx, acc_oe, 0, 0, 0);
                        acc_oo = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, by, acc_oo, 0, 0, 0);
                    }
                }
            }
            return;
        }
        // The stage straddles a pair boundary (a few dozen waves per launch): group the 8 records of each MFMA step by pair.
        // One copy of the code — the loop is kept rolled by rotating the stage's registers instead of indexing them.
        // (x and act are dead after this call: rotated in place)
        double2* y = x;
        uint32_t* a_ = act;
#pragma unroll 1
        for (int u = 0; u < U; ++u) {
            const bool ok = a_[0] & 1u;
            const double w = weight(y[0]);
            const int s = off + 8 * u + R;
            const bool in = s < len;
            const uint32_t key = in ? key0[s] : 0xFFFFFFFFu;
            unsigned long long remaining = __ballot(in);
            while (remaining) {
                const int first = __ffsll((long long)remaining) - 1;
                const uint32_t k0 = (uint32_t)__shfl((int)key, first);
                if (k0 != cur_key) {
                    if (dirty) flush();
                    cur_key = k0;
                    dirty = false;
                }
                const bool mine = in && (key == k0), use = mine && ok;
                if (__ballot(use)) {
                    dirty = true;
                    const double ax = use ? w * y[0].x : 0.0, ay = use ? w * y[0].y : 0.0, bx = use ? y[0].x : 0.0, by = use ? y[0].y : 0.0;
                    if (!EMBA_ABL(p.ablate, 64)) {
                        acc_ee = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, bx, acc_ee, 0, 0, 0);
                        acc_oe = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, bx, acc_oe, 0, 0, 0);
                        acc_oo = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, by, acc_oo, 0, 0, 0);
                    }
                }
                remaining &= ~__ballot(mine);
            }
#pragma unroll
            for (int v = 0; v + 1 < U; ++v) { y[v] = y[v + 1]; a_[v] = a_[v + 1]; }
        }
    };
    if constexpr (TAGS && SPARSE) {
        // SPARSE slot streams (10 M events on a 2048 x 4096 panorama in pixel order — 7 % of the slots live; the dense form gates ten million tags in
        // stages of 32 to fetch two records per stage, one memory latency per stage: 177-181 us at 1.6 TB/s; this form: 77-79 us).  A stage is 64 TS = 128 slots: TS coalesced
        // tag loads, TS activity gathers, TS ballots; the live slots' positions are compacted through a 128-byte LDS strip of the wave and only they are fetched — 8 U records
        // per round, all of a stage's in one round while fewer than 1 slot in 4 is live (more: further rounds on the spot).  Per stage the dependent steps tags -> activity
        // words -> records -> sums are spread over three iterations as in the dense form: while stage j-1 is summed, the records of stage j, the activity words of j+1 and
        // the tags of j+2 are in flight.  The pair keys of a stage's first and last slot bound those of every record in it (slots are sorted by pair): same fast path.
        __shared__ uint8_t s_pos[kGramBlock / 64][64 * TS];
        uint8_t* pos = s_pos[threadIdx.x >> 6];
        const double* tag0 = p.tag + start;
        const int tag_lim = (int)((p.n_slots + kGramPad - 1 - start < (long)0x7FFFFFF0) ? (p.n_slots + kGramPad - 1 - start) : (long)0x7FFFFFF0);
        typedef const uint32_t __attribute__((address_space(4))) * const_u32_ptr;
        const_u32_ptr key_s = (const_u32_ptr)(uintptr_t)key0;
        const double2* recm = reinterpret_cast<const double2*>(p.rec + (size_t)kRecStride * start) + m;      // + 8 s: piece m of the record in slot start + s
        auto tags = [&](int off, double* T) {
#pragma unroll
            for (int t = 0; t < TS; ++t) { const int sidx = off + 64 * t + lane; T[t] = tag0[sidx < tag_lim ? sidx : tag_lim]; }
        };
        auto words = [&](int off, const double* T, uint32_t* S, uint32_t* W) {      // S: bit 5 = the tag is this evaluation's, bits 0-4 = its pixel's bit in the activity word
#pragma unroll
            for (int t = 0; t < TS; ++t) {
                const uint32_t pi = (uint32_t)__double2loint(T[t]);
                const bool valid = off + 64 * t + lane < len && (uint32_t)__double2hiint(T[t]) == p.stamp && pi != kInvalidPix;
                S[t] = valid ? (32u | (pi & 31u)) : 0u;
                W[t] = p.active_bits[valid ? (pi >> 5) : 0u];                       // (unconditional: a load under a lane mask is waited for at the end of its branch)
            }
        };
        auto compact = [&](const uint32_t* S, const uint32_t* W) -> int {           // live slots of the stage -> pos[0 .. total)
            int total = 0;
#pragma unroll
            for (int t = 0; t < TS; ++t) {
                const bool live = (S[t] & 32u) && (((EMBA_ABL(p.ablate, 256) ? ~0u : W[t]) >> (S[t] & 31u)) & 1u);
                const unsigned long long M = __ballot(live);
                if (live) pos[total + __popcll(M & ((1ull << lane) - 1ull))] = (uint8_t)(64 * t + lane);
                total += (int)__popcll(M);
            }
            return total;
        };
        auto fetch = [&](int off, int total, int round, double2* x, int* sidx) {    // records pos[8 U round ..) of the stage at off
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = 8 * U * round + 8 * u + R;
                const bool v = q < total;
                const int sl = off + (int)pos[v ? q : 0];
                sidx[u] = v ? sl : -1;
                x[u] = v ? recm[8 * (size_t)sl] : make_double2(0.0, 0.0);
            }
        };
        auto consume_s = [&](double2* x, int* sidx) {
            if ((k_first == cur_key) && (k_last == cur_key)) {             // fast path: the whole stage belongs to the current pair
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool ok = sidx[u] >= 0;
                    const double w = weight(x[u]);
                    const double ax = ok ? w * x[u].x : 0.0, ay = ok ? w * x[u].y : 0.0, bx = ok ? x[u].x : 0.0, by = ok ? x[u].y : 0.0;
                    if (__ballot(ok)) {
                        dirty = true;
                        if (!EMBA_ABL(p.ablate, 64)) {
                            acc_ee = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, bx, acc_ee, 0, 0, 0);
                            acc_oe = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, bx, acc_oe, 0, 0, 0);
                            acc_oo = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, by, acc_oo, 0, 0, 0);
                        }
                    }
                }
                return;
            }
            // the stage straddles a pair boundary: the records of each MFMA step grouped by pair (rolled loop, registers rotated; x and sidx are dead after this call)
#pragma unroll 1
            for (int u = 0; u < U; ++u) {
                const bool in = sidx[0] >= 0;
                const double w = weight(x[0]);
                const uint32_t key = in ? key0[sidx[0]] : 0xFFFFFFFFu;
                unsigned long long remaining = __ballot(in);
                while (remaining) {
                    const int first = __ffsll((long long)remaining) - 1;
                    const uint32_t k0 = (uint32_t)__shfl((int)key, first);
                    if (k0 != cur_key) {
                        if (dirty) flush();
                        cur_key = k0;
                        dirty = false;
                    }
                    const bool mine = in && (key == k0);
                    dirty = true;
                    const double ax = mine ? w * x[0].x : 0.0, ay = mine ? w * x[0].y : 0.0, bx = mine ? x[0].x : 0.0, by = mine ? x[0].y : 0.0;
                    if (!EMBA_ABL(p.ablate, 64)) {
                        acc_ee = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, bx, acc_ee, 0, 0, 0);
                        acc_oe = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, bx, acc_oe, 0, 0, 0);
                        acc_oo = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, by, acc_oo, 0, 0, 0);
                    }
                    remaining &= ~__ballot(mine);
                }
#pragma unroll
                for (int v = 0; v + 1 < U; ++v) { x[v] = x[v + 1]; sidx[v] = sidx[v + 1]; }
            }
        };
        // iteration j (stage j at off): (a) the sums of stage j-1 — its first round is in xP, further rounds are fetched on the spot while its positions still stand —,
        // (b) stage j's live slots compacted and its first round of records requested, (c) activity words of stage j+1, (d) tags of stage j+2
        int totP = 0, offP = 0; uint32_t kfP = 0, klP = 0;
        double T[TS];                                            // tags: of stage j+1 at the top of iteration j (one register set: read by words(), then reloaded)
        auto iterate = [&](int off, double2* xP, int* sP, double2* xC, int* sC, const uint32_t* Sc, const uint32_t* Wc, uint32_t* Sn, uint32_t* Wn) {
            if (totP > 0) {
                k_first = kfP; k_last = klP;
                consume_s(xP, sP);
                for (int round = 1; 8 * U * round < totP; ++round) { fetch(offP, totP, round, xP, sP); consume_s(xP, sP); }
            }
            const int tot = (off < len) ? compact(Sc, Wc) : 0;
            if (tot > 0) {
                fetch(off, tot, 0, xC, sC);
                kfP = key_s[off]; klP = key_s[(off + kStage < len ? off + kStage : len) - 1];
            }
            totP = tot; offP = off;
            words(off + kStride, T, Sn, Wn);
            tags(off + 2 * kStride, T);
        };
        uint32_t Sa[TS], Sb[TS], Wa[TS], Wb[TS];
        double2 xA2[U], xB2[U]; int sA[U], sB[U];
        tags(off0, T);
        words(off0, T, Sa, Wa);
        tags(off0 + kStride, T);
        // stage j: S / W in (Sa, Wa) for even j, (Sb, Wb) for odd j; records of even stages in xA2, of odd stages in xB2.  One iteration past the last stage sums it.
        for (int off = off0; off - kStride < len;) {
            iterate(off, xB2, sB, xA2, sA, Sa, Wa, Sb, Wb); off += kStride; if (off - kStride >= len) break;
            iterate(off, xA2, sA, xB2, sB, Sb, Wb, Sa, Wa); off += kStride;
        }
    } else
    if (TAGS) {
        // Tag stream: one 8-B word {panorama pixel, evaluation stamp} per slot, written by the warp kernels next to the record.  A stage
        // first reads its 32 tags (256 contiguous bytes), looks the activity bits up, and then fetches ONLY the records that take part
        // (8 lanes = one 128-B line per record: a record that is stale, an outlier's, or on an inactive pixel is never read — about half
        // of the slots of the BASELINE workload).  Loads return in order, so the three dependent steps of a stage are spread over three
        // iterations: tags of stage i+2, activity bits of stage i+1 and records of stage i+1 are in flight while stage i is consumed.
        // What keeps the three steps apart in the generated code: tags and activity words are loaded UNCONDITIONALLY (clamped / safe
        // addresses, validity applied when the bit is extracted an iteration later), the pair keys come through the scalar cache, and
        // the two record buffers and the two tag registers alternate by an iteration unrolled twice — a conditional load is waited for
        // at the end of its branch, a vector key load or a copy of a register still being loaded waits for everything issued before it
        // (all three were the case: one stage's full latency per iteration).
        const double* tag0 = p.tag + start;
        const int tag_lim = (int)((p.n_slots + kGramPad - 1 - start < (long)0x7FFFFFF0) ? (p.n_slots + kGramPad - 1 - start) : (long)0x7FFFFFF0);
        auto tagload = [&](int off) -> double { const int sidx = off + lane; return tag0[sidx < tag_lim ? sidx : tag_lim]; };
        auto tagvalid = [&](int off, double tg) -> bool {
            return lane < 8 * U && off + lane < len && (uint32_t)__double2hiint(tg) == p.stamp && (uint32_t)__double2loint(tg) != kInvalidPix;
        };
        auto bitword = [&](int off, double tg) -> uint32_t { return p.active_bits[tagvalid(off, tg) ? ((uint32_t)__double2loint(tg) >> 5) : 0u]; };
        auto bitmask = [&](int off, double tg, uint32_t w) -> unsigned long long {   // one bit per slot of the stage (8 U <= 64 slots = lanes)
            const uint32_t bit = ((EMBA_ABL(p.ablate, 256) ? ~0u : w) >> ((uint32_t)__double2loint(tg) & 31u)) & (tagvalid(off, tg) ? 1u : 0u);
            return (unsigned long long)__ballot(bit != 0);
        };
        // (GRAM_DUMMY_LOADS: a record that does not take part is "loaded" from one fixed line instead — the block's first record, a cache
        // hit shared by all such lanes — so that the load is unconditional and the wait counts stay exact)
        const double2* dummy = reinterpret_cast<const double2*>(p.rec + (size_t)kRecStride * start) + (lane & 7);
        auto load_masked = [&](int off, unsigned long long m, double2* x) {
            const double2* q = rec0 + 8 * off;
#pragma unroll
            for (int u = 0; u < U; ++u) {
#if GRAM_DUMMY_LOADS
                x[u] = *(((m >> (8 * u + R)) & 1u) ? q + 64 * u : dummy);
#else
                if (GRAM_TAG_NT) {
                    typedef double v2d __attribute__((ext_vector_type(2)));
                    v2d v = {0.0, 0.0};
                    if ((m >> (8 * u + R)) & 1u) v = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(q + 64 * u));
                    x[u] = make_double2(v.x, v.y);
                } else
                x[u] = ((m >> (8 * u + R)) & 1u) ? q[64 * u] : make_double2(0.0, 0.0);
#endif
            }
        };
        typedef const uint32_t __attribute__((address_space(4))) * const_u32_ptr;
        const_u32_ptr key_s = (const_u32_ptr)(uintptr_t)key0;
        auto keys = [&](int off) { if constexpr (!PAIRED) { k_first = key_s[off]; k_last = key_s[(off + 8 * U < len ? off + 8 * U : len) - 1]; } };
        // iteration i: Tb = tags of stage i+1 (here), Tn = tags of stage i+2 (arriving), W = activity words of stage i+1 (arriving)
        static_assert(8 * U <= 64, "a stage's live mask is one wave ballot");
        unsigned long long Mc; uint32_t W;
        double Te, To;
        auto iterate = [&](int off, double2* cur, double2* nxt, double& Tb, double& Tn) {
            const bool h1 = off + kStride < len;
            const unsigned long long Mn = h1 ? bitmask(off + kStride, Tb, W) : 0ull;
            W = bitword(off + 2 * kStride, Tn);
            Tb = tagload(off + 3 * kStride);                 // (Tb's stage is done with: its register takes stage i+3)
            load_masked(h1 ? off + kStride : off, Mn, nxt);     // (Mn == 0 past the end: dummy loads only)
            keys(off);
#pragma unroll
            for (int u = 0; u < U; ++u) act[u] = (Mc >> (8 * u + R)) & 1u;
            if (Mc) consume(off, cur);
            Mc = Mn;
        };
        Te = tagload(off0);
        W = bitword(off0, Te);
        To = tagload(off0 + kStride);
        Mc = bitmask(off0, Te, W);
        W = bitword(off0 + kStride, To);
        Te = tagload(off0 + 2 * kStride);
        load_masked(off0, Mc, xA);
        for (int off = off0; off < len;) {
            iterate(off, xA, xB, To, Te); off += kStride; if (off >= len) break;
            iterate(off, xB, xA, Te, To); off += kStride;
        }
        // Tried and dropped (round 3, 1 M events): two record stages in flight per wave (three buffers of 24 records, tags / activity words
        // one step further ahead, stage 0 fetched unmasked beside its tags): 33.0 us against 30.9.  Ablation of the 30.9 us: the MFMAs
        // themselves ~4.7 (375 k v_mfma_f64_16x16x4 at 64 cycles on the chip's 1024 SIMDs is ~10 us of matrix-pipe time, half of it hidden),
        // the global flush ~3.7, the stream + its dependent start the remaining ~22.
    } else {
    // No tag stream (tile order): the activity bits of a stage can only be looked up once its records are here, and loads return in
    // order.  Four stages rotate through registers: per iteration the lookups of stage i+1 (whose records arrived an iteration ago)
    // are issued, then the records of stage i+3, and stage i is consumed — its lookups were issued one iteration earlier, AHEAD of
    // the record loads of stage i+2, so the wait for them leaves two stages of records in flight.  (Two stages, lookups in the
    // critical path: 3.15 ms for 12.7 GB at 100 M events; without the lookups 2.24 ms.)
    // The four stage buffers are used round-robin by an iteration unrolled four times — copying a register a load is still
    // in flight to would wait for that load.
    double2 xC[U], xD[U];
    uint32_t actB[U], kfA = 0, klA = 0, kfB = 0, klB = 0;
    // (pair keys through the scalar cache: as vector loads they would be waited for with every record load issued before them)
    typedef const uint32_t __attribute__((address_space(4))) * const_u32_ptr;
    const_u32_ptr key_s = (const_u32_ptr)(uintptr_t)key0;
    auto lookup_into = [&](int off, const double2* x, uint32_t* a, uint32_t& f, uint32_t& l) {
        f = key_s[off < len ? off : len - 1];                    // (a stage past the end is never consumed)
        l = key_s[(off + 8 * U < len ? off + 8 * U : len) - 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t pi = rec_elem15_lo(x[u]);
            const bool in = off + 8 * u + R < len;
            const bool valid = in && rec_elem15_hi(x[u]) == p.stamp && pi != kInvalidPix;
            // An UNCONDITIONAL load from a safe address: a load the compiler can sink under a lane mask is waited for at the end of
            // that branch, together with everything issued before it.  Only the raw word is kept: the bit is extracted when the
            // stage is consumed (an iteration later), so nothing here waits for the gather.
            a[u] = p.active_bits[valid ? (pi >> 5) : 0u];
        }
    };
    auto resolve = [&](int off, const double2* x, const uint32_t* w) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t pi = rec_elem15_lo(x[u]);
            const bool valid = (off + 8 * u + R < len) && rec_elem15_hi(x[u]) == p.stamp && pi != kInvalidPix;
            act[u] = ((EMBA_ABL(p.ablate, 256) ? ~0u : w[u]) >> (pi & 31)) & (valid ? 1u : 0u);
        }
    };
    // one iteration: stage i in `cur` (its lookups in a_cur / f_cur, l_cur), stage i+1 in `nxt`, stage i+3 goes to `fre`
    // (no load sits under a branch: stages past the block's end are fetched from a clamped, allocated offset and masked out — with
    // conditional loads the compiler's wait-count bookkeeping degrades to "wait for everything" at the joins)
    const int off_max = (int)((p.n_slots + kGramPad - 8 * U - start < (long)0x7FFFFFF0) ? (p.n_slots + kGramPad - 8 * U - start) : (long)0x7FFFFFF0);
    auto load_clamped = [&](int off, double2* x) { load_records(off < off_max ? off : off_max, x); };
    auto iterate = [&](int off, double2* cur, double2* nxt, double2* fre, uint32_t* a_cur, uint32_t f_cur, uint32_t l_cur, uint32_t* a_nxt,
                       uint32_t& f_nxt, uint32_t& l_nxt) {
        lookup_into(off + kStride, nxt, a_nxt, f_nxt, l_nxt);
        load_clamped(off + 3 * kStride, fre);
        k_first = f_cur; k_last = l_cur;
        resolve(off, cur, a_cur);
        consume(off, cur);
    };
    uint32_t actA[U];
    load_clamped(off0, xA);
    load_clamped(off0 + kStride, xB);
    load_clamped(off0 + 2 * kStride, xC);
    lookup_into(off0, xA, actA, kfA, klA);
    for (int off = off0; off < len;) {
        iterate(off, xA, xB, xD, actA, kfA, klA, actB, kfB, klB); off += kStride; if (off >= len) break;
        iterate(off, xB, xC, xA, actB, kfB, klB, actA, kfA, klA); off += kStride; if (off >= len) break;
        iterate(off, xC, xD, xB, actA, kfA, klA, actB, kfB, klB); off += kStride; if (off >= len) break;
        iterate(off, xD, xA, xC, actB, kfB, klB, actA, kfA, klA); off += kStride;
    }
    }
#if !GRAM_WAVE_TILE
    if (dirty) flush();
#else
    if (dirty) {      // the wave's last pair: plain stores into its own tile (a pair change in mid-stream — a few dozen waves per launch — went through flush())
        const int wabs = threadIdx.x >> 6;
        gram_wave_tile(acc_ee, acc_oe, acc_oo, s_wtile + wabs * 256);
        if (lane == 0) s_wkey[wabs] = cur_key;
    }
#endif
    }  // have_work
    __syncthreads();
    // block-level flush of the combine table: entry (k, row, col) by thread k*256 + row*16 + col
    if constexpr (!PAIRED)
    for (int i = threadIdx.x; i < kGramKeys * 256; i += kGramBlock) {
        const uint32_t key = s_tag[i >> 8];
        if (key != 0xFFFFFFFFu) gram_atomic_out(s_tile[i], (i >> 4) & 15, i & 15, key, p.A11, p.b1, p.dim, p.ablate);
    }
    // ... and of the waves' own tiles: thread e < 256 owns entry e; the waves that ended on the same pair are summed first (the first of them leads).
    // The sixteen keys come to registers in one go and every tile read is independent of the others (block-uniform predicates): two LDS round trips, not a
    // chain of a hundred (which cost this kernel 5 us when it was written as loops over LDS-resident keys).
    if (threadIdx.x < 256) {
        const int e = threadIdx.x, row = e >> 4, col = e & 15;
        constexpr int NW = kGramBlock / 64;
        uint32_t kw[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) kw[w] = s_wkey[w];
        double tv[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) tv[w] = (kw[w] != 0xFFFFFFFFu) ? s_wtile[w * 256 + e] : 0.0;
        if (row < 12 && (col < 12 || col == 14)) {
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                if (kw[w] == 0xFFFFFFFFu) continue;
                bool leader = true;
#pragma unroll
                for (int w2 = 0; w2 < w; ++w2) leader = leader && (kw[w2] != kw[w]);
                if (!leader) continue;
                double sum = 0.0;
#pragma unroll
                for (int w2 = w; w2 < NW; ++w2) sum += (kw[w2] == kw[w]) ? tv[w2] : 0.0;
                gram_atomic_out(sum, row, col, kw[w], p.A11, p.b1, p.dim, p.ablate);
            }
        }
    }
}

// ep = the inliers' residuals in the reference's order (model.cpp:221,256: sensor pixel major, then time = pm-order) — what evaluateDataError RETURNS.
// Round 5: in the resident step the compaction rides at the END of the Gram launch instead of being a scan + a compaction launch of
// its own (+ 10 us per step at 1 M events).  Launch A has left the inlier-flag count of every kFlagBlk pm entries; a tail block takes kEpTailBlk entries
// (four of those), sums the counts in front of it itself (L2-resident words) and
// writes its inliers' residuals at their ranks.  The tail blocks start as Gram blocks retire (one 16-wave block per CU either way).
constexpr int kEpTailBlk = 4 * kFlagBlk;
// Round 6: at every window length (round 5: up to 8.4 M entries, longer windows paid a one-block scan of all block counts — 101 us at 100 M events — and a compaction launch
// of 1024-entry blocks behind the Gram kernel).  The inliers in front of a tail block = launch A's super-counts (one word per kFlagSup block counts = 64 K entries) in front of
// it + the <= kFlagSup - 1 block counts behind the last whole super-count.
__device__ __forceinline__ void ep_tail_block(long cb, const GramParams& p)
{
    __shared__ uint32_t s_x[kGramBlock / 64], s_b[kGramBlock / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const long nfront = cb * (kEpTailBlk / kFlagBlk);
    const long nsup = nfront / kFlagSup;
    uint32_t part = 0;
    for (long s0 = 0; s0 < nsup; s0 += kGramBlock) { const long s = s0 + t; if (s < nsup) part += p.ep_fsup[s * kFlagSupStride]; }
    for (long j0 = nsup * kFlagSup; j0 < nfront; j0 += kGramBlock) {
        const long j = j0 + t;
        const uint32_t v = p.ep_fblk_cnt[j < p.ep_n_fblk ? j : p.ep_n_fblk - 1];
        if (j < nfront) part += v;
    }
    const long i0 = cb * kEpTailBlk + 4L * t;
    uint32_t fl = 0;
    double e[4] = {0.0, 0.0, 0.0, 0.0};
    if (i0 + 4 <= p.ep_n_pm) {
        fl = *reinterpret_cast<const uint32_t*>(p.ep_flag + i0);
        const double2 a = *reinterpret_cast<const double2*>(p.ep_e + i0), b = *reinterpret_cast<const double2*>(p.ep_e + i0 + 2);
        e[0] = a.x; e[1] = a.y; e[2] = b.x; e[3] = b.y;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (i0 + k < p.ep_n_pm) { fl |= (uint32_t)p.ep_flag[i0 + k] << (8 * k); e[k] = p.ep_e[i0 + k]; }
    }
    const uint32_t m = ((fl & 0xFFu) ? 1u : 0u) | ((fl & 0xFF00u) ? 2u : 0u) | ((fl & 0xFF0000u) ? 4u : 0u) | ((fl & 0xFF000000u) ? 8u : 0u);
    const uint32_t mine = __popc(m);
    uint32_t x = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o); if (lane >= o) x += y; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o);
    if (lane == 63) s_x[wv] = x;
    if (lane == 0) s_b[wv] = part;
    __syncthreads();
    uint32_t k = x - mine;
#pragma unroll
    for (int w = 0; w < kGramBlock / 64; ++w) { k += s_b[w]; if (w < wv) k += s_x[w]; }
#pragma unroll
    for (int q = 0; q < 4; ++q) if (m & (1u << q)) p.ep_out[k++] = e[q];
    // (round 6, measured and dropped: the block's inliers through 32 KB of LDS at their ranks and out in one coalesced sweep — city + 28 vs + 35 us, 40 M + 169 vs + 180,
    // 100 M + 453 vs + 460: the compaction moves 17 B per event at 3.7-4 TB/s either way, next to a Gram kernel that is itself bandwidth-bound)
}

template <bool TAGS, bool GATHER, bool SPARSE = false, bool PAIRED = false>
__global__ __launch_bounds__(kGramBlock) void emba_gram_kernel(GramParams p, ActiveWriteParams aw)
{
    if ((int)blockIdx.x >= p.n_gram_blocks) { ep_tail_block((long)blockIdx.x - p.n_gram_blocks, p); return; }      // (block-uniform)
    gram_body<TAGS, kGramBlock, GATHER, SPARSE, PAIRED>(p, blockIdx.x, aw);
}

// A22 / b2 from the records, for the weighted (IRLS) or caller-supplied-ep cases (model.cpp:599-636); the quadratic
// case takes them from pixacc instead.  One thread per record, five fp64 atomics into the compact pack.
__global__ void emba_a22_from_records_kernel(const double* __restrict__ rec, long n_slots, const int32_t* __restrict__ count,
                                             const int32_t* __restrict__ compact, int thres, int irls, double eta,
                                             double* __restrict__ A22b2, uint32_t stamp)
{
    const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    const double2* r2 = reinterpret_cast<const double2*>(rec + (size_t)kRecStride * s);
    const double2 tail = r2[7];
    uint32_t pi;
    if (!record_valid(tail.y, stamp, pi) || count[pi] < thres) return;
    const double e = tail.x;
    double w = 1.0;
    if (irls == 2) w = 1.0 / (1.0 + eta * e * e);
    else if (irls == 1) { const double a = fabs(e); w = (a < eta) ? 1.0 : eta / a; }
    const double ew = w * e;
    const double2 d = r2[6];
    double* q = A22b2 + 5 * (size_t)compact[pi];
    atomicAdd(q + 0, w * (d.x * d.x));
    atomicAdd(q + 1, w * (d.x * d.y));
    atomicAdd(q + 2, w * (d.y * d.y));
    atomicAdd(q + 3, d.x * ew);
    atomicAdd(q + 4, d.y * ew);
}

// a11: applyL2Reg (model.cpp:689-719) on the compact pack.
__global__ void emba_l2reg_kernel(double* __restrict__ A22b2, const uint32_t* __restrict__ active_idx, const uint32_t* __restrict__ P_dev,
                                  double alpha, const double* __restrict__ Gx, const double* __restrict__ Gy)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)P_dev[0]) return;   // P lives in device memory: the host may not have read it back yet
    double* q = A22b2 + 5 * i;
    const uint32_t pi = active_idx[i];
    q[0] += alpha;
    q[2] += alpha;
    q[3] -= alpha * Gx[pi];
    q[4] -= alpha * Gy[pi];
}

// f2: LEGM::updateMap (model.cpp:863-903) from the current map into the trial map.
__global__ void emba_update_map_kernel(const double* __restrict__ Gx, const double* __restrict__ Gy, const int32_t* __restrict__ compact,
                                       const double* __restrict__ x2, double damping, long npix, double* __restrict__ Gx_new,
                                       double* __restrict__ Gy_new)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int32_t k = compact[i];
    Gx_new[i] = (k >= 0) ? Gx[i] + damping * x2[2 * (size_t)k] : 0.0;         // :874 / :897
    Gy_new[i] = (k >= 0) ? Gy[i] + damping * x2[2 * (size_t)k + 1] : 0.0;     // :875 / :898
}

// the map at the active pixels only (emba_get_map_active): out[2k] = Gx[active_k], out[2k+1] = Gy[active_k]
__global__ void emba_map_active_kernel(const double* __restrict__ Gx, const double* __restrict__ Gy, const uint32_t* __restrict__ active_idx, long P,
                                       double* __restrict__ out)
{
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    const uint32_t i = active_idx[k];
    reinterpret_cast<double2*>(out)[k] = make_double2(Gx[i], Gy[i]);
}

// pack -> boundary layout: A22 P*4 ([xx xy; xy yy]) and b2 2P.
__global__ void emba_unpack_kernel(const double* __restrict__ A22b2, long P, double* __restrict__ A22, double* __restrict__ b2)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const double* q = A22b2 + 5 * i;
    A22[4 * i + 0] = q[0]; A22[4 * i + 1] = q[1]; A22[4 * i + 2] = q[1]; A22[4 * i + 3] = q[2];
    b2[2 * i] = q[3]; b2[2 * i + 1] = q[4];
}

// Weight and compact pixel of a record (shared by the dense-A12 and export kernels).
__device__ __forceinline__ bool record_active(const double* rec, const int32_t* count, const int32_t* compact, int thres,
                                              int irls, double eta, uint32_t stamp, int32_t* cidx, double* w)
{
    const double2 tail = reinterpret_cast<const double2*>(rec)[7];
    uint32_t pi;
    // (activity from the compact index of the active set, not from the count map: after a rejected LM trial the count map is the trial's)
    if (!record_valid(tail.y, stamp, pi) || compact[pi] < 0) return false;
    (void)count; (void)thres;
    const double e = tail.x;
    double ww = 1.0;
    if (irls == 2) ww = 1.0 / (1.0 + eta * e * e);
    else if (irls == 1) { const double a = fabs(e); ww = (a < eta) ? 1.0 : eta / a; }
    *cidx = compact[pi];
    *w = ww;
    return true;
}

// Dense A12 (3K x 2P col-major) for the legacy interface (model.cpp:358,483-487); small sizes only.
__global__ void emba_dense_a12_kernel(const double* __restrict__ rec, const uint32_t* __restrict__ slot_key, long n_slots,
                                      const int32_t* __restrict__ count, const int32_t* __restrict__ compact, int thres,
                                      int irls, double eta, int dim, double* __restrict__ A12, uint32_t stamp)
{
    const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    const double* r = rec + (size_t)kRecStride * s;
    int32_t cidx; double w;
    if (!record_active(r, count, compact, thres, irls, eta, stamp, &cidx, &w)) return;
    const uint32_t key = slot_key[s];
    const int bc = 3 * (int)(key >> 16), bp = 3 * (int)(key & 0xFFFFu);
    double* c0 = A12 + (size_t)dim * (2 * (size_t)cidx);
    double* c1 = c0 + dim;
    const double dx = r[12], dy = r[13];
    for (int i = 0; i < 6; ++i) {
        const double jc = w * r[i], jp = w * r[6 + i];
        atomicAdd(c0 + bc + i, jc * dx); atomicAdd(c1 + bc + i, jc * dy);
        atomicAdd(c0 + bp + i, jp * dx); atomicAdd(c1 + bp + i, jp * dy);
    }
}

// Sparse A12 export: one rank-1 factor per candidate slot.
__global__ void emba_export_a12_kernel(const double* __restrict__ rec, const uint32_t* __restrict__ slot_key, long n_slots,
                                       const int32_t* __restrict__ count, const int32_t* __restrict__ compact, int thres,
                                       int irls, double eta, int32_t* __restrict__ cp_c, int32_t* __restrict__ cp_p,
                                       int32_t* __restrict__ pix, double* __restrict__ w_out, double* __restrict__ jc,
                                       double* __restrict__ jp, double* __restrict__ dp, uint32_t stamp)
{
    const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    const double* r = rec + (size_t)kRecStride * s;
    const uint32_t key = slot_key[s];
    cp_c[s] = (int32_t)(key >> 16);
    cp_p[s] = (int32_t)(key & 0xFFFFu);
    int32_t cidx = -1; double w = 0.0;
    const bool ok = record_active(r, count, compact, thres, irls, eta, stamp, &cidx, &w);
    pix[s] = ok ? cidx : -1;
    w_out[s] = ok ? w : 0.0;
    for (int i = 0; i < 6; ++i) { jc[6 * s + i] = ok ? r[i] : 0.0; jp[6 * s + i] = ok ? r[6 + i] : 0.0; }
    dp[2 * s] = ok ? r[12] : 0.0; dp[2 * s + 1] = ok ? r[13] : 0.0;
}

__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// ------------------------------------------------------------------------------------------------
// Measurement aids of bench.py: what an event bracket around NOTHING reads on this box, and the shader clock the chip
// really runs at while it is busy.  Neither touches the product's data.
// ------------------------------------------------------------------------------------------------
__global__ void emba_empty_kernel() {}

constexpr int kClockProbeUnroll = 256;
// One wave per SIMD: a dependent chain of loops x kClockProbeUnroll v_add_f32 (a 16-lane SIMD issues a wave64 fp32 add in 4 cycles and dependent
// adds go back to back), bracketed by the constant-rate clock (s_memrealtime) and the shader's own counter (s_memtime).
// out[0] = s_memtime ticks, out[1] = s_memrealtime ticks (block 0, lane 0), out[2] = the chain's value (keeps it alive).
__global__ __launch_bounds__(256) void emba_clock_probe_kernel(unsigned long long* __restrict__ out, int loops)
{
    float x = (float)threadIdx.x, y = 1.0f;
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime(), t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < loops; ++i) {
#pragma unroll
        for (int u = 0; u < kClockProbeUnroll; ++u) __asm__ volatile("v_add_f32 %0, %0, %1" : "+v"(x) : "v"(y));
    }
    __asm__ volatile("s_nop 0" ::: "memory");
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (blockIdx.x == 0 && threadIdx.x == 0) { out[0] = t1 - t0; out[1] = r1 - r0; }
    if (x == -1.0f) out[2] = (unsigned long long)x;
}

}  // namespace emba
