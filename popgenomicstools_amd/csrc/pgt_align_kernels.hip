// pgt_align_kernels.hip — the sites common to K position columns, found on the device (pgt_sites_align), and the
// column gather that follows it (pgt_gather_dev).
//
// What is replaced: the two-file synchronisation of the reference's streaming loop (dxyWindow.cpp:315-331: one current
// line per file, the file that is behind reads on), generalised to K files as the intersection by (chromosome, position),
// which is what those loops produce on their defined domain.  The host names the matched chromosome
// segments of every file (pgt_align_segments); file 0 is the pivot:
//   1. align_match_kernel   one workgroup per tile of 1024 pivot rows (no tile straddles a segment; a lane holds 4 rows
//                           from one 16-byte load).  Per other file: the tile's first and last position are bracketed in
//                           that file's segment by a wave-cooperative search (64 probes per step); a bracket of at most
//                           8192 rows is staged in LDS (32 KiB, 16-byte loads) and every lane looks its positions up
//                           there, a longer one (files of very different density) is searched in global memory.  The
//                           rows found are parked in the workspace (file 1's slot doubles as the "in all files" flag);
//                           the tile's number of common sites goes to the tile table;
//   2. align_scan_kernel    exclusive prefix over the tile counts (one workgroup, as scan_blocks_kernel of the text
//                           ingest) + the first output row of every chromosome;
//   3. align_place_kernel   the same tiles again: rank of every common site inside its tile -> idx[k][first + rank].
// No atomics, no floating point: the index columns are a function of the inputs alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "pgt_device.h"
#include "pgt_internal.h"
#include "pgt_pops_common.h"  // hip_fail

namespace pgt {
namespace {

constexpr int kThreads = 256;
constexpr int kLaneRows = 4;
constexpr uint32_t kTile = kThreads * kLaneRows;  // pivot rows per workgroup
constexpr uint32_t kStage = 8192;                 // rows of another file a workgroup stages in LDS (32 KiB: five workgroups per CU)
constexpr uint32_t kNone = 0xFFFFFFFFu;           // "not in every file" (rows per file stay below 2^32 - 1)

struct AlignArgs {
    const uint32_t *pos[kAlignMaxFiles];
    uint32_t *prov[kAlignMaxFiles];  // [k][pivot row]: the row of the pivot's site in file k (k >= 1); prov[1]: kNone unless in all files
    uint32_t *idx[kAlignMaxFiles];
    uint32_t n_rows[kAlignMaxFiles];
    const uint2 *seg;            // [chromosome][file] {off, len}
    const uint32_t *tile_first;  // n_chr + 1: first tile of every chromosome
    uint32_t n_chr, n_files;
    uint32_t shift;              // (address of pos[0] / 4) mod 4: tiles start where a 16-byte load of the pivot is aligned
};

struct Tile {
    uint32_t chr;
    int64_t g0;       // pivot row of lane 0's first element (may lie up to 3 rows in front of the segment)
    uint32_t lo, hi;  // the tile's pivot rows [lo, hi), not empty
};

__device__ __forceinline__ Tile tile_of(const AlignArgs &a, uint32_t b) {
    uint32_t m = 0, e = a.n_chr;  // the last chromosome whose first tile is <= b (chromosomes without tiles are stepped over)
    while (e - m > 1) {
        const uint32_t mid = (m + e) >> 1;
        if (a.tile_first[mid] <= b) m = mid; else e = mid;
    }
    const uint2 s = a.seg[(size_t)m * a.n_files];
    Tile t;
    t.chr = m;
    t.g0 = (int64_t)s.x - (int64_t)((s.x + a.shift) & 3u) + (int64_t)(b - a.tile_first[m]) * kTile;
    t.lo = t.g0 > (int64_t)s.x ? (uint32_t)t.g0 : s.x;
    const uint64_t end = (uint64_t)s.x + s.y, te = (uint64_t)(t.g0 + kTile);
    t.hi = (uint32_t)(te < end ? te : end);
    return t;
}

// 4 consecutive u32 of `col` from row g: one 16-byte load where all four lie in [lo, hi) (g is then 16-byte aligned by
// the caller's construction), else row by row; rows outside read as `fill`
__device__ __forceinline__ void load4(const uint32_t *col, int64_t g, uint32_t lo, uint32_t hi, uint32_t fill, uint32_t v[4]) {
    if (g >= (int64_t)lo && g + 4 <= (int64_t)hi) {
        const uint4 w = *reinterpret_cast<const uint4 *>(col + g);
        v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (g + j >= (int64_t)lo && g + j < (int64_t)hi) ? col[g + j] : fill;
    }
}

// First row r of col[lo, hi) (strictly increasing) with col[r] >= key (UPPER: > key); hi if none.  The whole wave calls
// it with the same arguments: every step probes 64 rows, one per lane, and keeps the gap the answer lies in.
template <bool UPPER>
__device__ __forceinline__ uint32_t wave_bound(const uint32_t *col, uint32_t lo, uint32_t hi, uint32_t key, int lane) {
    while (hi > lo) {
        const uint32_t stride = (hi - lo + 63u) / 64u;
        const uint64_t q = (uint64_t)lo + (uint64_t)lane * stride;
        bool before = false;
        if (q < hi) {
            const uint32_t x = col[q];
            before = UPPER ? x <= key : x < key;
        }
        const uint32_t c = (uint32_t)__popcll(__ballot(before));  // the probes are ordered: a prefix of the lanes
        if (c == 0) return lo;
        const uint64_t last = (uint64_t)lo + (uint64_t)(c - 1) * stride;
        lo = (uint32_t)(last + 1);
        hi = (uint32_t)(last + stride < hi ? last + stride : hi);
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void align_match_kernel(AlignArgs a, uint32_t *tile_count) {
    __shared__ __attribute__((aligned(16))) uint32_t stage[kStage + 8];
    __shared__ uint32_t bracket[kAlignMaxFiles][2];
    __shared__ uint32_t wave_count[kThreads / kWave];
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const Tile t = tile_of(a, blockIdx.x);
    const int64_t g = t.g0 + (int64_t)tid * kLaneRows;
    uint32_t p[4];
    load4(a.pos[0], g, t.lo, t.hi, 0, p);
    uint32_t alive = 0;  // bit j: row g + j is a pivot row of this tile and still in every file looked at
#pragma unroll
    for (int j = 0; j < 4; ++j) alive |= (uint32_t)(g + j >= (int64_t)t.lo && g + j < (int64_t)t.hi) << j;
    const uint32_t mine = alive;

    // brackets: wave w takes the files 1 + w, 5 + w
    const uint32_t p_first = a.pos[0][t.lo], p_last = a.pos[0][t.hi - 1];
    for (uint32_t k = 1 + (uint32_t)wave; k < a.n_files; k += kThreads / kWave) {
        const uint2 s = a.seg[(size_t)t.chr * a.n_files + k];
        const uint32_t b_lo = wave_bound<false>(a.pos[k], s.x, s.x + s.y, p_first, lane);
        const uint32_t b_hi = wave_bound<true>(a.pos[k], b_lo, s.x + s.y, p_last, lane);
        if (lane == 0) { bracket[k][0] = b_lo; bracket[k][1] = b_hi; }
    }
    __syncthreads();

    uint32_t r1[4] = {kNone, kNone, kNone, kNone};
    for (uint32_t k = 1; k < a.n_files; ++k) {
        const uint32_t *col = a.pos[k];
        const uint32_t b_lo = bracket[k][0], b_hi = bracket[k][1];
        const bool in_lds = b_hi - b_lo <= kStage;
        // staged rows [s0, ...): s0 = b_lo rounded down to a 16-byte boundary of the column
        const int64_t s0 = (int64_t)b_lo - (int64_t)((b_lo + (uint32_t)((reinterpret_cast<uintptr_t>(col) >> 2) & 3u)) & 3u);
        if (in_lds) {
            const uint32_t chunks = (uint32_t)(((int64_t)b_hi - s0 + 3) / 4);  // <= (kStage + 3 + 3) / 4
            for (uint32_t c = (uint32_t)tid; c < chunks; c += kThreads) {
                uint32_t v[4];
                load4(col, s0 + 4 * (int64_t)c, 0, a.n_rows[k], 0, v);
                *reinterpret_cast<uint4 *>(&stage[4 * c]) = make_uint4(v[0], v[1], v[2], v[3]);
            }
            __syncthreads();
        }
        uint32_t r[4];
        uint32_t from = b_lo;  // a lane's positions increase: each search starts where the last one ended
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[j] = kNone;
            if (!((alive >> j) & 1u)) continue;
            uint32_t l = from, h = b_hi;
            bool hit;
            if (in_lds) {
                while (l < h) {
                    const uint32_t mid = l + ((h - l) >> 1);
                    if (stage[(int64_t)mid - s0] < p[j]) l = mid + 1; else h = mid;
                }
                hit = l < b_hi && stage[(int64_t)l - s0] == p[j];
            } else {
                while (l < h) {
                    const uint32_t mid = l + ((h - l) >> 1);
                    if (col[mid] < p[j]) l = mid + 1; else h = mid;
                }
                hit = l < b_hi && col[l] == p[j];
            }
            from = l;
            if (hit) r[j] = l; else alive &= ~(1u << j);
        }
        if (k == 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) r1[j] = r[j];
        } else if (mine == 15u) {
            *reinterpret_cast<uint4 *>(a.prov[k] + g) = make_uint4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((mine >> j) & 1u) a.prov[k][g + j] = r[j];
        }
        if (in_lds) __syncthreads();  // the next file overwrites the stage
    }
    // file 1's slot carries the verdict of all files
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (!((alive >> j) & 1u)) r1[j] = kNone;
    if (mine == 15u) {
        *reinterpret_cast<uint4 *>(a.prov[1] + g) = make_uint4(r1[0], r1[1], r1[2], r1[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((mine >> j) & 1u) a.prov[1][g + j] = r1[j];
    }
    const uint32_t c = dev::wave_sum((uint32_t)__popc(alive));
    if (lane == 0) wave_count[wave] = c;
    __syncthreads();
    if (tid == 0) tile_count[blockIdx.x] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
}

// one workgroup: first[i] = sum of count[0 .. i), chr_first[m] = first output row of chromosome m, chr_first[n_chr] = total
__global__ __launch_bounds__(1024) void align_scan_kernel(const uint32_t *count, uint64_t *first, uint32_t n, const uint32_t *tile_first,
                                                          uint64_t *chr_first, uint32_t n_chr) {
    __shared__ uint64_t part[1024];
    __shared__ uint64_t total;
    const uint32_t per = (n + 1023u) / 1024u;
    const uint64_t lo = (uint64_t)per * threadIdx.x, hi = lo + per < n ? lo + per : n;
    uint64_t s = 0;
    for (uint64_t i = lo; i < hi; ++i) s += count[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (int t = 0; t < 1024; ++t) { const uint64_t v = part[t]; part[t] = run; run += v; }
        total = run;
    }
    __syncthreads();
    uint64_t run = part[threadIdx.x];
    for (uint64_t i = lo; i < hi; ++i) { first[i] = run; run += count[i]; }
    __syncthreads();  // first[] of this workgroup's own stores is read below
    for (uint32_t m = threadIdx.x; m <= n_chr; m += 1024) chr_first[m] = tile_first[m] < n ? first[tile_first[m]] : total;
}

__global__ __launch_bounds__(kThreads) void align_place_kernel(AlignArgs a, const uint64_t *tile_row, uint64_t cap) {
    __shared__ uint32_t wave_count[kThreads / kWave];
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const Tile t = tile_of(a, blockIdx.x);
    const int64_t g = t.g0 + (int64_t)tid * kLaneRows;
    uint32_t r1[4];
    load4(a.prov[1], g, t.lo, t.hi, kNone, r1);  // prov[k] + g is aligned as pos[0] + g is
    uint32_t common = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) common |= (uint32_t)(r1[j] != kNone) << j;
    const uint32_t c = (uint32_t)__popc(common);
    uint32_t incl = c;  // inclusive prefix over the wave
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d, kWave);
        if (lane >= d) incl += up;
    }
    if (lane == kWave - 1) wave_count[wave] = incl;
    __syncthreads();
    uint64_t o = tile_row[blockIdx.x] + (incl - c);
    for (int w = 0; w < wave; ++w) o += wave_count[w];
    if (c == 0) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!((common >> j) & 1u)) continue;
        if (o < cap) {
            a.idx[0][o] = (uint32_t)(g + j);
            a.idx[1][o] = r1[j];
            for (uint32_t k = 2; k < a.n_files; ++k) a.idx[k][o] = a.prov[k][g + j];
        }
        ++o;
    }
}

// dst[m] = src[idx[m]]: a lane takes 4 consecutive outputs (idx by one 16-byte load, 16-byte stores) where `vec` says that
// idx and dst are 16-byte aligned; idx increases, so a wave's loads fall into few cache lines
template <class T>
__global__ __launch_bounds__(kThreads) void gather_kernel(T *dst, const T *src, const uint32_t *idx, uint64_t n, int vec) {
    const uint64_t i = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
    if (i >= n) return;
    if (vec && i + 4 <= n) {
        const uint4 ix = *reinterpret_cast<const uint4 *>(idx + i);
        const T v0 = src[ix.x], v1 = src[ix.y], v2 = src[ix.z], v3 = src[ix.w];
        if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<uint4 *>(dst + i) = make_uint4(v0, v1, v2, v3);
        } else {
            *reinterpret_cast<ulonglong2 *>(dst + i) = make_ulonglong2(v0, v1);
            *reinterpret_cast<ulonglong2 *>(dst + i + 2) = make_ulonglong2(v2, v3);
        }
    } else {
        for (uint64_t j = i; j < n && j < i + 4; ++j) dst[j] = src[idx[j]];
    }
}

size_t pad256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

AlignLayout align_layout(uint32_t n_files, uint64_t n_rows_file0) {
    AlignLayout l{};
    l.max_tiles = n_rows_file0 / kTile + 2 * (uint64_t)kAlignMaxChr + 1;  // a segment of L rows: at most L / 1024 + 2 tiles
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += pad256(bytes); return at; };
    l.seg = take((size_t)kAlignMaxChr * n_files * sizeof(uint2));
    l.tile_first = take(((size_t)kAlignMaxChr + 1) * sizeof(uint32_t));
    l.chr_first = take(((size_t)kAlignMaxChr + 1) * sizeof(uint64_t));
    l.tile_count = take(l.max_tiles * sizeof(uint32_t));
    l.tile_row = take(l.max_tiles * sizeof(uint64_t));
    for (uint32_t k = 1; k < n_files; ++k) l.prov[k] = take((n_rows_file0 + 8) * sizeof(uint32_t));
    l.bytes = off;
    return l;
}

int launch_sites_align(const uint32_t *const *pos, const uint64_t *n_rows, uint32_t n_files, const pgt_seg *seg, size_t n_chr,
                       uint32_t *const *idx, uint64_t cap, uint64_t *seg_count, uint64_t *n_common, void *work, void *stream,
                       std::string *err) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const AlignLayout l = align_layout(n_files, n_rows[0]);
    char *w = static_cast<char *>(work);
    AlignArgs a{};
    a.n_chr = (uint32_t)n_chr;
    a.n_files = n_files;
    a.shift = (uint32_t)((reinterpret_cast<uintptr_t>(pos[0]) >> 2) & 3u);
    for (uint32_t k = 0; k < n_files; ++k) {
        a.pos[k] = pos[k];
        a.idx[k] = idx[k];
        a.n_rows[k] = (uint32_t)n_rows[k];
        a.prov[k] = k ? reinterpret_cast<uint32_t *>(w + l.prov[k]) + a.shift : nullptr;
    }
    a.seg = reinterpret_cast<const uint2 *>(w + l.seg);
    a.tile_first = reinterpret_cast<const uint32_t *>(w + l.tile_first);

    // the plan: segments as u32 pairs, first tile of every chromosome
    std::vector<uint2> h_seg(n_chr * n_files);
    std::vector<uint32_t> h_first(n_chr + 1, 0);
    for (size_t m = 0; m < n_chr; ++m) {
        for (uint32_t k = 0; k < n_files; ++k) h_seg[m * n_files + k] = make_uint2((uint32_t)seg[m * n_files + k].off, (uint32_t)seg[m * n_files + k].len);
        const uint64_t off = seg[m * n_files].off, len = seg[m * n_files].len;
        const uint64_t a0 = off - ((off + a.shift) & 3u);  // (wraps for off < 3: only the difference below is used)
        h_first[m + 1] = h_first[m] + (uint32_t)(len ? (off + len - a0 + kTile - 1) / kTile : 0);
    }
    const uint32_t n_tiles = h_first[n_chr];
    *n_common = 0;
    for (size_t m = 0; m < n_chr; ++m) seg_count[m] = 0;
    if (n_tiles == 0) return PGT_OK;
    if (n_tiles > l.max_tiles) {
        if (err) *err = "pgt_sites_align: internal error: more tiles than the workspace holds";
        return PGT_EARG;
    }
    if (int rc = hip_fail(hipMemcpyAsync(w + l.seg, h_seg.data(), h_seg.size() * sizeof(uint2), hipMemcpyHostToDevice, s), "pgt_sites_align: segment upload", err)) return rc;
    if (int rc = hip_fail(hipMemcpyAsync(w + l.tile_first, h_first.data(), h_first.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s), "pgt_sites_align: tile plan upload", err)) return rc;
    uint32_t *tile_count = reinterpret_cast<uint32_t *>(w + l.tile_count);
    uint64_t *tile_row = reinterpret_cast<uint64_t *>(w + l.tile_row);
    uint64_t *chr_first = reinterpret_cast<uint64_t *>(w + l.chr_first);
    hipLaunchKernelGGL(align_match_kernel, dim3(n_tiles), dim3(kThreads), 0, s, a, tile_count);
    if (int rc = hip_fail(hipGetLastError(), "align_match_kernel", err)) return rc;
    hipLaunchKernelGGL(align_scan_kernel, dim3(1), dim3(1024), 0, s, tile_count, tile_row, n_tiles, a.tile_first, chr_first, a.n_chr);
    if (int rc = hip_fail(hipGetLastError(), "align_scan_kernel", err)) return rc;
    std::vector<uint64_t> h_chr(n_chr + 1);
    if (int rc = hip_fail(hipMemcpyAsync(h_chr.data(), chr_first, h_chr.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s), "pgt_sites_align: count download", err)) return rc;
    if (int rc = hip_fail(hipStreamSynchronize(s), "pgt_sites_align: hipStreamSynchronize", err)) return rc;
    *n_common = h_chr[n_chr];
    for (size_t m = 0; m < n_chr; ++m) seg_count[m] = h_chr[m + 1] - h_chr[m];
    if (*n_common && cap) {  // rows beyond cap are not written
        hipLaunchKernelGGL(align_place_kernel, dim3(n_tiles), dim3(kThreads), 0, s, a, tile_row, cap);
        if (int rc = hip_fail(hipGetLastError(), "align_place_kernel", err)) return rc;
        if (int rc = hip_fail(hipStreamSynchronize(s), "pgt_sites_align: hipStreamSynchronize", err)) return rc;
    }
    return PGT_OK;
}

int launch_gather(void *dst, const void *src, const uint32_t *idx, uint64_t n, uint32_t elem_bytes, void *stream, std::string *err) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) return PGT_OK;
    const int vec = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(idx)) & 15u) == 0;
    const uint64_t blocks = (n + kTile - 1) / kTile;
    if (elem_bytes == 4)
        hipLaunchKernelGGL(gather_kernel<uint32_t>, dim3((unsigned)blocks), dim3(kThreads), 0, s, static_cast<uint32_t *>(dst),
                           static_cast<const uint32_t *>(src), idx, n, vec);
    else
        hipLaunchKernelGGL(gather_kernel<unsigned long long>, dim3((unsigned)blocks), dim3(kThreads), 0, s, static_cast<unsigned long long *>(dst),
                           static_cast<const unsigned long long *>(src), idx, n, vec);
    return hip_fail(hipGetLastError(), "gather_kernel", err);
}

}  // namespace pgt
