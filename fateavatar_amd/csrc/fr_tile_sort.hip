// Depth sort of each 8x8 tile's list for gfx950: the ordering the reference gets from one device-wide radix sort of
// (tile | depth) keys and identifyTileRanges (rasterizer_impl.cu:300-318).  The binning has already put a tile's keys into
// the tile's own buckets, so every list is sorted on its own, by depth alone.
//
// Execution model: a bitonic network in registers, across lanes and registers.  One wave sorts a list of up to 256 keys,
// four waves one of up to 2 048 (k_tile_sort) or 4 096 (k_tile_sort_big, on a side stream) with three exchanges through
// LDS; longer lists take a network over global memory.  What a list's sorter leaves is the Gaussian id of every key in
// blend order (BinningView::ids); k_tile_sort also writes the descriptors and hand-off words of the tile's blend units and
// the frame's verdict and counts.
#include "fr_tile.hpp"

namespace fr {

// Where a tile's unsorted keys live: eight per-XCD buckets (ImageView::buckets), sub-list x starting at position
// sub[x] of the tile's list.  key(i) = i-th key of the tile in that concatenation order.
struct KeySrc {
    const u64* base;     // bucket of XCD 0 of this tile
    uint32_t cap;        // keys per bucket
    uint32_t sub[kXcds]; // start of every XCD's sub-list (sub[0] == 0)
    __device__ __forceinline__ u64 key(uint32_t i) const
    {
        uint32_t x = 0;
#pragma unroll
        for (int k = 1; k < kXcds; k++) x += (i >= sub[k]) ? 1u : 0u;   // sub[] ascends: x = last sub-list starting at or before i
        uint32_t s0 = sub[0];
#pragma unroll
        for (int k = 1; k < kXcds; k++) s0 = (x == (uint32_t)k) ? sub[k] : s0;
        return base[(size_t)x * cap + (i - s0)];
    }
};
__device__ __forceinline__ KeySrc key_src(const ImageView& v, uint32_t tile)
{
    KeySrc ks;
    ks.base = reinterpret_cast<const u64*>(v.buckets) + (size_t)tile * kXcds * v.bucket_cap;
    ks.cap = v.bucket_cap;
    const uint4 a = *reinterpret_cast<const uint4*>(v.tile_sub + (size_t)tile * kSubWords);
    const uint4 b = *reinterpret_cast<const uint4*>(v.tile_sub + (size_t)tile * kSubWords + 4);
    ks.sub[0] = a.x, ks.sub[1] = a.y, ks.sub[2] = a.z, ks.sub[3] = a.w;
    ks.sub[4] = b.x, ks.sub[5] = b.y, ks.sub[6] = b.z, ks.sub[7] = b.w;
    return ks;
}

__device__ __forceinline__ u64 umin64(u64 a, u64 b) { return a < b ? a : b; }
__device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a < b ? b : a; }

// ---- bitonic network, "flip" formulation (every compare-exchange puts the smaller key at the lower index).
// A wave holds 64 K keys, K per lane: ELEMENT e = lane * K + r (the 4-wave variants: + 64 K * wave).  The lane index carries the
// high bits, so the short exchange distances — 1 .. K/2, which every merge level ends with — are exchanges between a lane's
// own registers (a compare and four selects per pair, no cross-lane move), and only distances of K and more go through DPP /
// ds_swizzle / v_permlane32_swap.  (Until round 6 the layout was e = r * 64 + lane: every distance below 64 was a cross-lane
// exchange — 35 cross-lane stages and one register stage for 256 keys, against 21 and 15 now; one wave's 256 keys 4.1 -> 3 us.)
// A stage exchanges e with e ^ M: lane ^ (M / K) and register ^ (M & (K - 1)).
template <int K, int LM, int LOWBIT, int RM>
__device__ __forceinline__ void lane_stage(u64 (&v)[K], int lane)
{
    // partner = (lane ^ LM, register ^ RM); this lane holds the lower index iff (lane & LOWBIT) == 0
    const bool lower = (lane & LOWBIT) == 0;
    u64 b[K];
#pragma unroll
    for (int r = 0; r < K; r++) b[r] = lane_xor_u64<LM>(v[r ^ RM], lane);
#pragma unroll
    for (int r = 0; r < K; r++) v[r] = ((v[r] < b[r]) == lower) ? v[r] : b[r];   // keep the min (lower lane) / the max (upper lane)
}
template <int K, int JR>
__device__ __forceinline__ void reg_stage(u64 (&v)[K])
{
    // pairs (r, r ^ JR) of a lane's own registers: the smaller key to the lower register
#pragma unroll
    for (int r = 0; r < K; r++) {
        const int rp = r ^ JR;
        if (rp > r) {
            const u64 a = v[r], b = v[rp];
            v[r] = umin64(a, b);
            v[rp] = umax64(a, b);
        }
    }
}
// half-cleaners at element distances J, J/2, ..., 1
template <int K, int J>
__device__ __forceinline__ void cleaners_from(u64 (&v)[K], int lane)
{
    if constexpr (J >= 1) {
        if constexpr (J >= K) lane_stage<K, J / K, J / K, 0>(v, lane);
        else reg_stage<K, J>(v);
        cleaners_from<K, J / 2>(v, lane);
    }
}
// one merge level: blocks of KK elements (flip with e ^ (KK - 1), then the half-cleaners KK/4 ... 1)
template <int K, int KK>
__device__ __forceinline__ void merge_level(u64 (&v)[K], int lane)
{
    if constexpr (KK <= K) reg_stage<K, KK - 1>(v);
    else lane_stage<K, KK / K - 1, KK / K / 2, K - 1>(v, lane);
    cleaners_from<K, KK / 4>(v, lane);
}
template <int K, int KK>
__device__ __forceinline__ void merge_levels_up_to(u64 (&v)[K], int lane)
{
    if constexpr (KK >= 2) {
        merge_levels_up_to<K, KK / 2>(v, lane);
        merge_level<K, KK>(v, lane);
    }
}
// the cleaners behind a cross-wave stage: element distances 32 K ... 1 inside the wave
template <int K>
__device__ __forceinline__ void wave_cleaners(u64 (&v)[K], int lane)
{
    cleaners_from<K, 32 * K>(v, lane);
}

// one wave sorts 64*K keys (K = 1, 2, 4, 8, 16)
template <int K>
__device__ __forceinline__ void wave_sort(u64 (&v)[K], int lane)
{
    merge_levels_up_to<K, 64 * K>(v, lane);
}

// The sort's output: the Gaussian id of every sorted key (slot r of lane l is list position base + l*K + r); the blend
// kernels gather the records themselves (RecSrc).
template <int K>
__device__ __forceinline__ void write_ids(uint32_t* ids, uint32_t start, uint32_t n, uint32_t base, const u64 (&v)[K], int lane)
{
#pragma unroll
    for (int r = 0; r < K; r++) {
        const uint32_t i = base + (uint32_t)(lane * K + r);   // (K consecutive ids per lane)
        if (i < n) ids[start + i] = (uint32_t)v[r];
    }
}

template <int K>
__device__ __forceinline__ void sort_tile_regs(const KeySrc& keys, uint32_t* ids, uint32_t start, uint32_t n, int lane)
{
    u64 v[K];
#pragma unroll
    for (int r = 0; r < K; r++) {
        const uint32_t i = (uint32_t)(lane * K + r);
        v[r] = i < n ? keys.key(i) : ~0ull;
    }
    wave_sort<K>(v, lane);
    write_ids<K>(ids, start, n, 0u, v, lane);
}

// Four waves sort up to 4 * 64 * K keys together (K = 4: 1024, K = 16: 4096): each wave sorts its 64*K keys in
// registers, then the two remaining merge levels exchange registers with the partner wave through LDS
// (3 exchanges in total).
template <int K>
struct SortXchgT {
    u64 a[4][K][64];
    __device__ __forceinline__ u64 (&operator[](int w))[K][64] { return a[w]; }
};

template <int K, bool FLIP>
__device__ __forceinline__ void cross_wave_stage(u64 (&v)[K], SortXchgT<K>& sx,int wave, int lane, int pw, bool lower)
{
    __syncthreads();
#pragma unroll
    for (int r = 0; r < K; r++) sx[wave][r][lane] = v[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < K; r++) {
        const u64 b = FLIP ? sx[pw][r ^ (K - 1)][lane ^ 63] : sx[pw][r][lane];
        v[r] = ((v[r] < b) == lower) ? v[r] : b;
    }
}

template <int K>
__device__ void sort_tile_group(const KeySrc& keys, uint32_t* ids, uint32_t start, uint32_t n, int wave, int lane, SortXchgT<K>& sx)
{
    constexpr int KW = 64 * K;  // keys per wave
    u64 v[K];
#pragma unroll
    for (int r = 0; r < K; r++) {
        const uint32_t i = (uint32_t)(wave * KW + lane * K + r);
        v[r] = i < n ? keys.key(i) : ~0ull;
    }
    wave_sort<K>(v, lane);
    // blocks of 2*KW: flip with wave ^ 1 (element e ^ (KW - 1): lane ^ 63, register ^ (K - 1)), then the distances inside the wave
    cross_wave_stage<K, true>(v, sx, wave, lane, wave ^ 1, (wave & 1) == 0);
    wave_cleaners<K>(v, lane);
    // blocks of 4*KW: flip with wave ^ 3, distance KW with wave ^ 1, then inside the wave
    cross_wave_stage<K, true>(v, sx, wave, lane, wave ^ 3, (wave & 2) == 0);
    cross_wave_stage<K, false>(v, sx, wave, lane, wave ^ 1, (wave & 1) == 0);
    wave_cleaners<K>(v, lane);
    write_ids<K>(ids, start, n, (uint32_t)(wave * KW), v, lane);
}

// Slow path for a tile list longer than kSortRegMax: bitonic network over the tile's key segment
// in global memory by one 256-thread workgroup (virtual +inf padding: a compare-exchange whose
// upper index is >= n is a no-op in the flip formulation).  Agent-scope accesses keep the data
// out of the per-CU L1 so that waves of the workgroup see each other's stores.
__device__ void sort_tile_global(const KeySrc& src, u64* keys, uint32_t* ids, uint32_t start, uint32_t n)
{
    u64* seg = keys + start;   // contiguous scratch segment of the tile inside the binning buffer
    uint32_t N = 1;
    while (N < n) N <<= 1;
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    for (uint32_t i = tid; i < n; i += nt) __hip_atomic_store(seg + i, src.key(i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    auto stage = [&](uint32_t mask) {
        for (uint32_t i = tid; i < N; i += nt) {
            const uint32_t p = i ^ mask;
            if (p > i && p < n) {
                const u64 a = __hip_atomic_load(seg + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const u64 b = __hip_atomic_load(seg + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (b < a) {
                    __hip_atomic_store(seg + i, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(seg + p, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        __syncthreads();
    };
    for (uint32_t k = 2; k <= N; k <<= 1) {
        stage(k - 1);                                    // flip
        for (uint32_t j = k >> 2; j >= 1; j >>= 1) stage(j);  // half-cleaners
    }
    for (uint32_t i = tid; i < n; i += nt) {
        const u64 kv = __hip_atomic_load(seg + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ids[start + i] = (uint32_t)kv;
    }
}

// The frame's verdict, from the cursors k_tile_totals left: too many instances for the record capacity, or a
// (tile, XCD) list longer than its key bucket.
__device__ __forceinline__ bool frame_overflow(const DeviceCounts* c, uint32_t bucket_cap)
{
    return c->num_instances > c->capacity || c->max_bucket > bucket_cap;
}

// Grid: kMediumSorters workgroups that sort the medium lists (257..2048 keys, four waves per list, static
// round-robin over the list k_tile_totals built), followed by Q = ceil(T/4) workgroups of 4 waves for the
// short lists: wave w of workgroup b owns tile w*Q + b (strided, so that the dense neighbouring tiles of one
// image region land in different workgroups) and sorts it in registers if it has <= 256 keys.  Lists longer
// than 2048 are left to k_tile_sort_big.
#ifndef FR_MEDIUM_SORTERS
#define FR_MEDIUM_SORTERS 1024
#endif
constexpr uint32_t kMediumSorters = FR_MEDIUM_SORTERS;  // workgroups that sort the medium lists while the others sort the short ones

struct SortArgs {
    ImageView v;
    uint32_t T, Q;
    u64* keys;
    uint32_t* ids;
    uint4* unit_tile;
    uint32_t unit_cap;
    float* unit_tseg;
    int take_long_lists;
    fr_counts* host_counts;
    uint32_t* unit_done;
    float* empty_color;
    const float* bg;
    int W, H;
    uint32_t* stripe_cursor;
};

// PLANES (FR_FLAG_DEPTH_ALPHA): a tile without instances also gets depth 0 and alpha 0 in out_depth / out_alpha.
template <bool PLANES>
__device__ __forceinline__ void tile_sort_body(const SortArgs& a, float* __restrict__ out_depth, float* __restrict__ out_alpha)
{
    const ImageView v = a.v;
    const uint32_t T = a.T, Q = a.Q, unit_cap = a.unit_cap;
    u64* keys = a.keys;
    uint32_t* ids = a.ids;
    uint4* unit_tile = a.unit_tile;
    float* unit_tseg = a.unit_tseg;
    const int take_long_lists = a.take_long_lists, W = a.W, H = a.H;
    fr_counts* host_counts = a.host_counts;
    uint32_t* unit_done = a.unit_done;
    float* empty_color = a.empty_color;
    const float* __restrict__ bg = a.bg;
    __shared__ SortXchgT<8> sx8;   // (16 KB: the exchange buffer of the longest lists this kernel sorts, 2 048 keys)
    SortXchgT<4>& sx = *reinterpret_cast<SortXchgT<4>*>(&sx8);
    const bool overflow = frame_overflow(v.counts, v.bucket_cap);
    if (blockIdx.x == 0 && threadIdx.x < 2 * kStripes) a.stripe_cursor[threadIdx.x * kStripeWords] = 0u;   // (BwdUnit list cursors)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the frame's verdict for the later kernels, and the counts for the host (pinned memory; made visible by the
        // end-of-kernel release; word 4 of the 64-byte slot = largest bucket need)
        DeviceCounts* c = v.counts;
        c->overflow = overflow ? 1u : 0u;
        host_counts->num_rendered = c->num_rendered;
        host_counts->num_instances = c->num_instances;
        host_counts->max_tile_list = c->max_tile_list;
        host_counts->overflow = overflow ? 1u : 0u;
        reinterpret_cast<uint32_t*>(host_counts)[4] = c->max_bucket;
        reinterpret_cast<uint32_t*>(host_counts)[5] = overflow ? 0u : c->num_units;   // (sizes the blend backward's grid)
        if (overflow) c->num_units = 0u;   // nothing to blend
    }
    // longest jobs first in dispatch order: medium lists, then the short ones
    if (blockIdx.x < kMediumSorters) {
        if (overflow) return;
        // medium lists (<= 2048): four waves each, static round-robin over the list built by k_tile_totals
        const int lane = threadIdx.x & 63;
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const uint32_t nm = v.counts->medium_tiles;
        SortXchgT<2>& sx2 = *reinterpret_cast<SortXchgT<2>*>(&sx);   // (lists up to 512: half the network)
        for (uint32_t item = blockIdx.x; item < nm; item += kMediumSorters) {
            const uint32_t tile = v.medium_list[item];
            const uint32_t n = v.tile_total[tile];
            // (the lane and the wave index are laundered once per item: otherwise every lane-dependent address and predicate of
            // the three networks below is hoisted out of this loop — which normally runs once — and held in registers for the
            // kernel's whole life)
            int ln = lane, wv = wave;
            asm volatile("" : "+v"(ln), "+s"(wv));
            if (n <= 512u) sort_tile_group<2>(key_src(v, tile), ids, v.tile_offset[tile], n, wv, ln, sx2);
            else if (n <= 1024u) sort_tile_group<4>(key_src(v, tile), ids, v.tile_offset[tile], n, wv, ln, sx);
            else sort_tile_group<8>(key_src(v, tile), ids, v.tile_offset[tile], n, wv, ln, sx8);   // (<= kSortGroupMax = 2 048)
        }
        // Lists longer than 2048 normally go to k_tile_sort_big.  When the host has not launched it (the previous
        // frame had no such list: one launch less per frame) any that turn up are still sorted here, by the slow
        // global-memory network — correct, just not fast; the next frame gets the big sorter back.
        if (take_long_lists) {
            const uint32_t nb = v.counts->big_tiles, nl = v.counts->large_tiles;
            for (uint32_t item = blockIdx.x; item < nb + nl; item += kMediumSorters) {
                const uint32_t tile = item < nb ? v.big_list[item] : v.large_list[item - nb];
                sort_tile_global(key_src(v, tile), keys, ids, v.tile_offset[tile], v.tile_total[tile]);
            }
        }
        return;
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    {
        const uint32_t tile = (uint32_t)wave * Q + (blockIdx.x - kMediumSorters);
        if (blockIdx.x - kMediumSorters < Q && tile < T) {   // (a batched launch's grid is the largest view's)
            // (everything the tile's wave reads before its keys — list start and length, first unit, sub-list table — in ONE
            // round trip, together with the frame's counts: none of it sits behind a branch on another load)
            const uint32_t start = v.tile_offset[tile];
            const uint32_t n = v.tile_total[tile];
            const uint32_t u0 = v.unit_offset[tile];
            const KeySrc ks = key_src(v, tile);
            asm volatile("" ::"s"(ks.sub[1]), "s"(ks.sub[7]), "s"(start), "s"(n), "s"(u0));
            if (overflow) return;   // (k_tile_totals has already zeroed the counters for the next frame)
            // descriptors of the tile's blend units (tile, segment, list start, list length): one coalesced store
            const uint32_t nu = (n + kUnit - 1) / kUnit;
            for (uint32_t k = (uint32_t)lane; k < nu; k += 64)
                if (u0 + k < unit_cap)   // (tile position, not tile index: the blend kernels need no division)
                    unit_tile[u0 + k] = make_uint4((tile / (uint32_t)v.tiles_x) << 16 | (tile % (uint32_t)v.tiles_x), k, start, n);
            // hand-off words of k_unit_blend_chained: a unit's per-pixel product is valid once it is non-zero
            if (unit_tseg)
                for (uint32_t k = 0; k + 1 < nu && u0 + k < unit_cap; k++) unit_tseg[(size_t)(u0 + k) * kUnit + lane] = 0.f;
            if (unit_done)
                for (uint32_t k = (uint32_t)lane; k < nu; k += 64)
                    if (u0 + k < unit_cap) unit_done[u0 + k] = 0u;
            // a tile without instances has no blend unit to write its pixels (gather-in-chain mode): background here
            if (empty_color && n == 0) {
                const int px = (int)(tile % (uint32_t)v.tiles_x) * kTile + (lane & 7);
                const int py = (int)(tile / (uint32_t)v.tiles_x) * kTile + (lane >> 3);
                if (px < W && py < H) {
                    const size_t pix = (size_t)py * W + px, HW = (size_t)H * W;
                    v.final_T[pix] = 1.0f;
                    v.n_contrib[pix] = 0u;
                    empty_color[pix] = bg[0], empty_color[HW + pix] = bg[1], empty_color[2 * HW + pix] = bg[2];
                    if (PLANES) out_depth[pix] = 0.f, out_alpha[pix] = 0.f;
                }
            }
            if (n > 0 && n <= (uint32_t)kSortWaveMax) {
                if (n <= 64) sort_tile_regs<1>(ks, ids, start, n, lane);
                else if (n <= 128) sort_tile_regs<2>(ks, ids, start, n, lane);
                else sort_tile_regs<4>(ks, ids, start, n, lane);
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_tile_sort(SortArgs a) { tile_sort_body<false>(a, nullptr, nullptr); }
__global__ void __launch_bounds__(256) k_tile_sort_batch(BatchOf<SortArgs> b) { tile_sort_body<false>(b.v[blockIdx.y], nullptr, nullptr); }
// frames with depth and alpha planes (FR_FLAG_DEPTH_ALPHA)
struct SortPlanesArgs {
    SortArgs s;
    float* out_depth;
    float* out_alpha;
};
__global__ void __launch_bounds__(256) k_tile_sort_planes(SortPlanesArgs a) { tile_sort_body<true>(a.s, a.out_depth, a.out_alpha); }
__global__ void __launch_bounds__(256) k_tile_sort_planes_batch(BatchOf<SortPlanesArgs> b)
{
    tile_sort_body<true>(b.v[blockIdx.y].s, b.v[blockIdx.y].out_depth, b.v[blockIdx.y].out_alpha);
}

// Lists longer than kSortGroupMax (dense / zoomed-in scenes): 4 waves x 16 keys per lane up to 4096, the
// global-memory network beyond.  A separate kernel so that its register budget (16 keys per lane) does not
// lower the occupancy of the common path.
constexpr uint32_t kBigSorters = 512;

struct BigSortArgs {
    ImageView v;
    u64* keys;
    uint32_t* ids;
};

__device__ __forceinline__ void tile_sort_big_body(const BigSortArgs& a)
{
    const ImageView v = a.v;
    u64* keys = a.keys;
    uint32_t* ids = a.ids;
    __shared__ SortXchgT<16> sx;
    SortXchgT<8>& sx8 = *reinterpret_cast<SortXchgT<8>*>(&sx);   // (lists up to 2048: half the network)
    if (frame_overflow(v.counts, v.bucket_cap)) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nb = v.counts->big_tiles, nl = v.counts->large_tiles;
    for (uint32_t item = blockIdx.x; item < nb; item += kBigSorters) {
        const uint32_t tile = v.big_list[item];
        const uint32_t n = v.tile_total[tile];
        if (n <= 2048u) sort_tile_group<8>(key_src(v, tile), ids, v.tile_offset[tile], n, wave, lane, sx8);
        else sort_tile_group<16>(key_src(v, tile), ids, v.tile_offset[tile], n, wave, lane, sx);
    }
    for (uint32_t item = blockIdx.x; item < nl; item += kBigSorters) {
        const uint32_t tile = v.large_list[item];
        sort_tile_global(key_src(v, tile), keys, ids, v.tile_offset[tile], v.tile_total[tile]);
    }
}

__global__ void __launch_bounds__(256) k_tile_sort_big(BigSortArgs a) { tile_sort_big_body(a); }
__global__ void __launch_bounds__(256) k_tile_sort_big_batch(BatchOf<BigSortArgs> b) { tile_sort_big_body(b.v[blockIdx.y]); }

int launch_tile_sort(int n, const FrameView* f, hipStream_t s, bool debug)
{
    fr_handle_impl* h0 = f[0].h;
    const bool planes = (f[0].prm->flags & FR_FLAG_DEPTH_ALPHA) != 0;   // (the same for every view of a batch)
    SortArgs sa[kMaxBatch];
    BigSortArgs ba[kMaxBatch];
    SortPlanesArgs sp[kMaxBatch];
    uint32_t sort_blocks = 0;
    // The big sorter is only launched when the most recent frame whose counts have reached the host had a list
    // longer than kSortGroupMax (or none has been seen yet); otherwise k_tile_sort keeps a slow but correct path for them.
    // (A batch launches it if any of its views asks for it.)
    bool launch_big = false;
    for (int k = 0; k < n; k++) {
        fr_handle_impl* h = f[k].h;
        launch_big = launch_big || !h->counts_seen || h->host_counts->max_tile_list > (uint32_t)kSortGroupMax;
        // (launch_blend_forward's condition, refused here: nothing of the frame's sort is enqueued for such a batch)
        if (n > 1 && (!h->gather_in_chain || h->gather_in_chain != h0->gather_in_chain))
            return fail_msg(FR_ERR_UNSUPPORTED, "batched frames need the gather inside the forward blend (unset FR_BLEND_FWD)");
    }
    for (int k = 0; k < n; k++) {
        fr_handle_impl* h = f[k].h;
        const fr_params& prm = *f[k].prm;
        const ImageView& v = f[k].v;
        const BinningView& b = f[k].b;
        const uint32_t T = (uint32_t)v.tiles_x * v.tiles_y;
        const uint32_t small_blocks = (T + 3) / 4;
        sort_blocks = max(sort_blocks, small_blocks + kMediumSorters);
        SortArgs& a = sa[k];
        a.v = v, a.T = T, a.Q = small_blocks, a.keys = (u64*)b.keys, a.ids = b.ids, a.unit_tile = b.unit_tile;
        a.unit_cap = (uint32_t)b.unit_cap, a.unit_tseg = b.unit_tseg, a.take_long_lists = launch_big ? 0 : 1;
        a.host_counts = h->host_counts_dev;
        a.unit_done = h->gather_in_chain ? b.unit_done : nullptr;
        a.empty_color = h->gather_in_chain ? f[k].out_color : nullptr;
        a.bg = f[k].in->background, a.W = prm.W, a.H = prm.H, a.stripe_cursor = b.stripe_cursor;
        ba[k].v = v, ba[k].keys = (u64*)b.keys, ba[k].ids = b.ids;
        if (planes) sp[k] = SortPlanesArgs{a, f[k].out_depth, f[k].out_alpha};
    }
    {
        StageScope sc(h0, ST_SORT, s);
        // the big sorter runs NEXT TO k_tile_sort, on the (first view's) handle's side stream: its few long lists take as long as
        // all the short ones together (config 5: 48 us against 65), the two kernels touch different tiles
        if (launch_big) {
            FR_HIP(hipEventRecord(h0->side_fork, s));
            FR_HIP(hipStreamWaitEvent(h0->side_stream, h0->side_fork, 0));
            launch_views(k_tile_sort_big, k_tile_sort_big_batch, n, ba, kBigSorters, 256, 0, h0->side_stream);
            FR_HIP(hipEventRecord(h0->side_join, h0->side_stream));
        }
        if (planes) launch_views(k_tile_sort_planes, k_tile_sort_planes_batch, n, sp, sort_blocks, 256, 0, s);
        else launch_views(k_tile_sort, k_tile_sort_batch, n, sa, sort_blocks, 256, 0, s);
        // the counts reach the pinned host slots with this kernel: the (waiting) forward blocks on them, not on the frame
        for (int k = 0; k < n; k++)
            if (!(f[k].prm->flags & FR_FLAG_NO_WAIT)) FR_HIP(hipEventRecord(f[k].h->counts_ready, s));
        if (launch_big) FR_HIP(hipStreamWaitEvent(s, h0->side_join, 0));
    }
    FR_HIP(hipGetLastError());
    return debug_sync(debug, s, "tile_sort");
}

}  // namespace fr
