// pgt_build_experiments.inc — what the tuning build adds to the product kernels (included by pgt_kernels_tuning.hip inside
// namespace pgt; the product build never compiles this file).  Pruned in round 4 to what a tool still uses:
//   fst_build_stamped_kernel   the product fst build with four s_memrealtime stamps per wave (tools/wave_timeline.py): where the
//                              fixed cost of a launch goes
//   launch_fst_experiment      the product kernel template with other parameters (PGT_TUNE_FST), for tools/build_ab.py and
//                              tools/size_sweep.py
//   fst_build_pair_kernel      round 4: two waves per level-2 tile (PGT_TUNE_FST_PAIR); +2-3 % at 1e8 sites, nothing on average
//   fst_build_ablate_kernel   round 7, timing only: the fst build without level-1 stores / without any flush in mid-stream
//                              (PGT_TUNE_FST_ABLATE): the prize of the deep node stage, profiles/r07/fst_deep_stage_prize.md
// (Round 4 also tried handing tiles out by an atomic ticket counter after a static first round — a loss at every size, see
// profiles/HISTORY.md and profiles/r04/ticket_schedule_rejected.patch.)
// The round-1/2/3 variants that lived here (straight, software-pipelined, store-wave, LDS-DMA ring, interleaved a/b, phased
// columns, one launch per stage) were measured and rejected or became the product; their code is in the history (last in
// commit 2192f93), their results under profiles/r01-r03 and in profiles/HISTORY.md.

// ------------------------------------------------------------------------------------------
// Four timestamps per wave (s_memrealtime, 100 MHz): start, first tile done, last tile done (before the final flush), end;
// + tiles taken + XCD / hardware id.  PGT_TUNE_BUILD_STAMPS=<file>: every launch is followed by a synchronous copy of the
// stamps to <file> (uint64 [n_waves][6] behind uint64 n_waves, n_tiles, double kernel ms).
// ------------------------------------------------------------------------------------------
template <int STAGE, int UNROLL>
__global__ __launch_bounds__(256) void fst_build_stamped_kernel(PairCols cols, uint64_t n, uint64_t n_l2, TreeView tv, uint64_t *stamps) {
    extern __shared__ __attribute__((aligned(16))) char lds_stage[];
    const int lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const double *__restrict__ a = cols.a[blockIdx.y];
    const double *__restrict__ b = cols.b[blockIdx.y];
    char *tree = tv.base + (size_t)blockIdx.y * tv.pair_stride;
    NodeFst *__restrict__ l1 = reinterpret_cast<NodeFst *>(tree + tv.off[0]);
    NodeFst *__restrict__ l2 = reinterpret_cast<NodeFst *>(tree + tv.off[1]);
    constexpr uint64_t kTile2 = (uint64_t)kLeafF64 * kRadix;
    NodeStage<NodeFst, STAGE, true> stage(lds_stage, wib, lane, l1, l2, n_waves);
    const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
    uint64_t t_first = 0, t_last = 0, done = 0;
    for (uint64_t t = wave0; t < n_l2; t += n_waves) {
        const uint64_t base = t * kTile2;
        double keep_a = 0.0, keep_b = 0.0;
        if (base + kTile2 <= n) {
            const double2 *__restrict__ pa = reinterpret_cast<const double2 *>(a + base);
            const double2 *__restrict__ pb = reinterpret_cast<const double2 *>(b + base);
#pragma unroll 1
            for (int j = 0; j < kRadix; j += UNROLL) {
                double2 v[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) v[u] = load16<true>(pa + (j + u) * kWave + lane);
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const double sa = wave_sum(v[u].x + v[u].y);
                    if (lane == j + u) keep_a = sa;
                }
            }
#pragma unroll 1
            for (int j = 0; j < kRadix; j += UNROLL) {
                double2 v[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) v[u] = load16<true>(pb + (j + u) * kWave + lane);
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const double sb = wave_sum(v[u].x + v[u].y);
                    if (lane == j + u) keep_b = sb;
                }
            }
        } else {
            for (int j = 0; j < kRadix; ++j) {
                const uint64_t i0 = base + (uint64_t)j * kLeafF64 + 2 * lane;
                if (base + (uint64_t)j * kLeafF64 >= n) break;  // wave-uniform
                const double a0 = i0 < n ? a[i0] : 0.0, a1 = i0 + 1 < n ? a[i0 + 1] : 0.0;
                const double b0 = i0 < n ? b[i0] : 0.0, b1 = i0 + 1 < n ? b[i0 + 1] : 0.0;
                const double sa = wave_sum(a0 + a1);
                const double sb = wave_sum(b0 + b1);
                if (lane == j) { keep_a = sa; keep_b = sb; }
            }
        }
        stage.put(t, NodeFst{keep_a, keep_b});
        t_last = __builtin_amdgcn_s_memrealtime();
        if (t_first == 0) t_first = t_last;
        ++done;
    }
    stage.flush();
    __builtin_amdgcn_s_waitcnt(0);  // the node stores have left the wave
    const uint64_t t_end = __builtin_amdgcn_s_memrealtime();
    if (lane == 0) {
        uint64_t *o = stamps + 6 * (wave0 + (uint64_t)blockIdx.y * n_waves);
        unsigned xcc = 0;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        unsigned hwid = 0;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        o[0] = t_start; o[1] = t_first; o[2] = t_last; o[3] = t_end; o[4] = done; o[5] = ((uint64_t)xcc << 32) | hwid;
    }
}

inline void launch_stamped(hipStream_t s, const PairCols &cols, uint32_t np, uint64_t n, uint64_t n_l2, const TreeView &tv, const char *path) {
    const unsigned blocks = build_grid(n_l2, kFstBuildBlocks);
    const uint64_t n_waves = (uint64_t)blocks * 4 * np;
    static uint64_t *d_stamps = nullptr;
    static uint64_t cap = 0;
    if (n_waves > cap) {
        if (d_stamps) (void)hipFree(d_stamps);
        (void)hipMalloc(reinterpret_cast<void **>(&d_stamps), n_waves * 6 * sizeof(uint64_t));
        cap = n_waves;
    }
    auto kernel = fst_build_stamped_kernel<kFstStage, 4>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFstStageBytes);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, s);
    hipLaunchKernelGGL(kernel, dim3(blocks, np), dim3(256), kFstStageBytes, s, cols, n, n_l2, tv, d_stamps);
    (void)hipEventRecord(e1, s);
    (void)hipStreamSynchronize(s);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    std::vector<uint64_t> h(n_waves * 6 + 3);
    h[0] = n_waves; h[1] = n_l2;
    double msd = ms;
    __builtin_memcpy(&h[2], &msd, 8);
    (void)hipMemcpy(h.data() + 3, d_stamps, n_waves * 6 * sizeof(uint64_t), hipMemcpyDeviceToHost);
    if (FILE *fp = std::fopen(path, "wb")) {
        std::fwrite(h.data(), sizeof(uint64_t), h.size(), fp);
        std::fclose(fp);
    }
}

// ------------------------------------------------------------------------------------------
// Round 4 experiment: TWO waves per level-2 tile.  A tile's 64 leaves are split between the two waves of a pair (leaves 0-31 /
// 32-63: 32 KiB of `a`, then 32 KiB of `b` each, still one column at a time), the 64 leaf nodes meet in the pair's LDS stage row
// and leave deferred as before; the level-2 node is the same 64-lane butterfly over the row — bits unchanged.  A workgroup (two
// pairs) takes two tiles per round behind one barrier, so a wave's work item is HALF a tile: twice the rounds, half the drain
// granularity, without undeferred rows (what sank the half-tile experiment of round 3).  PGT_TUNE_FST_PAIR=<loads in flight>.
// ------------------------------------------------------------------------------------------
template <int STAGE, int UNROLL>
__global__ __launch_bounds__(256) void fst_build_pair_kernel(PairCols cols, uint64_t n, uint64_t n_l2, TreeView tv) {
    extern __shared__ __attribute__((aligned(16))) char lds_stage[];
    const int lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6, pair = wib >> 1, half = wib & 1;
    const uint64_t pair0 = (uint64_t)blockIdx.x * 2 + pair, n_pairs = (uint64_t)gridDim.x * 2;
    const double *__restrict__ a = cols.a[blockIdx.y];
    const double *__restrict__ b = cols.b[blockIdx.y];
    char *tree = tv.base + (size_t)blockIdx.y * tv.pair_stride;
    NodeFst *__restrict__ l1 = reinterpret_cast<NodeFst *>(tree + tv.off[0]);
    NodeFst *__restrict__ l2 = reinterpret_cast<NodeFst *>(tree + tv.off[1]);
    constexpr uint64_t kTile2 = (uint64_t)kLeafF64 * kRadix;
    NodeFst *rows = reinterpret_cast<NodeFst *>(lds_stage) + (size_t)pair * STAGE * kWave;  // the pair's stage: [STAGE][64]
    int held = 0;
    uint64_t first_t = 0;
    auto flush = [&]() {  // by the pair's first wave; row k holds tile first_t + k * n_pairs
        if (half == 0)
            for (int k = 0; k < held; ++k) {
                const uint64_t t = first_t + (uint64_t)k * n_pairs;
                const NodeFst v = rows[k * kWave + lane];
                store_node_nt(&l1[t * kRadix + lane], v);
                const NodeFst top = node_wave_sum(v);
                if (lane == 0) l2[t] = top;
            }
        held = 0;
    };
    const uint64_t iters = (n_l2 + n_pairs - 1) / n_pairs;  // the same for every wave of the grid: the barriers below are uniform
    for (uint64_t it = 0; it < iters; ++it) {
        const uint64_t t = pair0 + it * n_pairs;
        const bool live = t < n_l2;
        if (live) {
            const uint64_t base = t * kTile2;
            double keep_a = 0.0, keep_b = 0.0;
            if (base + kTile2 <= n) {
                const double2 *__restrict__ pa = reinterpret_cast<const double2 *>(a + base);
                const double2 *__restrict__ pb = reinterpret_cast<const double2 *>(b + base);
                const int j0 = half * (kRadix / 2);
#pragma unroll 1
                for (int j = j0; j < j0 + kRadix / 2; j += UNROLL) {
                    double2 v[UNROLL];
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) v[u] = load16<true>(pa + (j + u) * kWave + lane);
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {
                        const double sa = wave_sum(v[u].x + v[u].y);
                        if (lane == j + u) keep_a = sa;
                    }
                }
#pragma unroll 1
                for (int j = j0; j < j0 + kRadix / 2; j += UNROLL) {
                    double2 v[UNROLL];
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) v[u] = load16<true>(pb + (j + u) * kWave + lane);
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {
                        const double sb = wave_sum(v[u].x + v[u].y);
                        if (lane == j + u) keep_b = sb;
                    }
                }
                if ((lane >> 5) == half) rows[held * kWave + lane] = NodeFst{keep_a, keep_b};
            } else if (half == 0) {  // the last, partial tile: the pair's first wave alone, as the product does it
                for (int j = 0; j < kRadix; ++j) {
                    const uint64_t i0 = base + (uint64_t)j * kLeafF64 + 2 * lane;
                    if (base + (uint64_t)j * kLeafF64 >= n) break;  // wave-uniform
                    const double a0 = i0 < n ? a[i0] : 0.0, a1 = i0 + 1 < n ? a[i0 + 1] : 0.0;
                    const double b0 = i0 < n ? b[i0] : 0.0, b1 = i0 + 1 < n ? b[i0 + 1] : 0.0;
                    const double sa = wave_sum(a0 + a1);
                    const double sb = wave_sum(b0 + b1);
                    if (lane == j) { keep_a = sa; keep_b = sb; }
                }
                rows[held * kWave + lane] = NodeFst{keep_a, keep_b};
            }
            if (held == 0) first_t = t;
            ++held;
        }
        __syncthreads();  // both halves of the row are in LDS
        if (held == STAGE) flush();
        __syncthreads();  // the rows may be overwritten
    }
    flush();
}

// ------------------------------------------------------------------------------------------
// Round 7, TIMING ONLY (the trees are wrong on purpose): what the mid-stream node flushes of a long column cost.
//   MODE 1  NodeStage without the level-1 row stores (round 6's ablation: profiles/r06/round6_c_ab_af_leaf_sizes_and_fst_store_share.md)
//   MODE 2  no flush in mid-stream at all: the rows that arrive while the kFstStage LDS rows are full are dropped, the rows held
//           leave in the one flush after the wave's last tile — the most a stage that never flushes in mid-stream can gain
//           (it writes 16 of 60 rows per wave at 10^9 sites; FstDeepStage writes them all)
// PGT_TUNE_FST_ABLATE=<mode>; profiles/r07/fst_deep_stage_prize.md.
// ------------------------------------------------------------------------------------------
template <int MODE>
struct AblateStage {
    NodeStage<NodeFst, kFstStage, true> inner;
    __device__ __forceinline__ AblateStage(char *lds, int wib, int lane, NodeFst *l1, NodeFst *l2, uint64_t n_waves)
        : inner(lds, wib, lane, l1, l2, n_waves) {}
    __device__ __forceinline__ void flush() {
        if (MODE == 2) return inner.flush();
        for (int k = 0; k < inner.held; ++k) {
            const uint64_t t = inner.first_t + (uint64_t)k * inner.n_waves;
            const NodeFst top = node_wave_sum(inner.rows[k * kWave + inner.lane]);
            if (inner.lane == 0) inner.l2[t] = top;
        }
        inner.held = 0;
    }
    __device__ __forceinline__ void put(uint64_t t, const NodeFst &keep) {
        if (MODE == 2 && inner.held == kFstStage) return;  // dropped
        if (inner.held == 0) inner.first_t = t;
        inner.rows[inner.held * kWave + inner.lane] = keep;
        ++inner.held;
        if (MODE == 1 && inner.held == kFstStage) flush();
    }
};
template <int MODE>
__global__ __launch_bounds__(256) void fst_build_ablate_kernel(PairCols cols, uint64_t n, uint64_t n_l2, TreeView tv) {
    extern __shared__ __attribute__((aligned(16))) char lds_stage[];
    fst_build_body<AblateStage<MODE>, 4, 4, 0>(PGT_BUILD_WAVE(), cols, n, n_l2, tv, lds_stage);
}

// Returns true when an experimental launch replaced the product's fst build.
//   PGT_TUNE_FST_ABLATE=1|2                                                   the timing-only kernels above
//   PGT_TUNE_FST_DEEP=1                                                       the deep-stage kernel at any size
//   PGT_TUNE_BUILD_STAMPS=<file>                                              the stamped copy
//   PGT_TUNE_FST=<stage>:<loads in flight>:<workgroups>[:<tail loads>:<tail scope>]   the product kernel template with other
//                parameters; tail scope 2 = a wave's whole last tile with <tail loads> in flight, 1 = its `b` column only
inline bool launch_fst_experiment(hipStream_t s, const PairCols &cols, uint32_t np, uint64_t n, const TreeLayout &tl, const TreeView &tv) {
    const uint64_t n_l2 = tl.count[1];
    if (const char *path = std::getenv("PGT_TUNE_BUILD_STAMPS")) {
        launch_stamped(s, cols, np, n, n_l2, tv, path);
        return true;
    }
    if (const char *e = std::getenv("PGT_TUNE_FST_ABLATE")) {
        auto go = [&](auto kernel) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFstStageBytes);
            hipLaunchKernelGGL(kernel, dim3(build_grid(n_l2, kFstBuildBlocks), np), dim3(256), kFstStageBytes, s, cols, n, n_l2, tv);
        };
        if (std::atoi(e) == 2) go(fst_build_ablate_kernel<2>);
        else go(fst_build_ablate_kernel<1>);
        return true;
    }
    if (std::getenv("PGT_TUNE_FST_DEEP")) {  // (its LDS attribute is set by init_kernels)
        hipLaunchKernelGGL(fst_build_kernel_deep, dim3(build_grid(n_l2, kFstBuildBlocks), np), dim3(256), kFstDeepStageBytes, s, cols, n, n_l2, tv);
        return true;
    }
    if (const char *e = std::getenv("PGT_TUNE_FST_PAIR")) {
        const uint64_t max_pairs = (uint64_t)kFstBuildBlocks * 2;  // 512 workgroups of two pairs
        const uint64_t rounds = (n_l2 + max_pairs - 1) / max_pairs, pairs = (n_l2 + rounds - 1) / rounds;
        const dim3 grid((unsigned)((pairs + 1) / 2), np);
        auto go = [&](auto kernel) {
            const size_t shmem = kFstStageBytes;  // the pairs need half of it; asking for all of it keeps two workgroups per CU
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
            hipLaunchKernelGGL(kernel, grid, dim3(256), shmem, s, cols, n, n_l2, tv);
        };
        if (std::atoi(e) == 8) go(fst_build_pair_kernel<16, 8>);
        else if (std::atoi(e) == 2) go(fst_build_pair_kernel<16, 2>);
        else go(fst_build_pair_kernel<16, 4>);
        return true;
    }
    if (const char *e = std::getenv("PGT_TUNE_FST")) {
        int stage = 16, unroll = 4, blocks = 512, tail = 0, scope = 0;
        std::sscanf(e, "%d:%d:%d:%d:%d", &stage, &unroll, &blocks, &tail, &scope);
        auto go = [&](auto kernel, int st) {
            const size_t shmem = (size_t)4 * st * 1024;
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
            hipLaunchKernelGGL(kernel, dim3(build_grid(n_l2, (unsigned)blocks), np), dim3(256), shmem, s, cols, n, n_l2, tv);
        };
        if (scope && unroll == 4 && tail == 8) { if (scope == 2) go(fst_build_kernel<16, 4, true, 8, 2>, 16); else go(fst_build_kernel<16, 4, true, 8, 1>, 16); }
        else if (scope && unroll == 4 && tail == 16) { if (scope == 2) go(fst_build_kernel<16, 4, true, 16, 2>, 16); else go(fst_build_kernel<16, 4, true, 16, 1>, 16); }
        else if (stage == 16 && unroll == 8) go(fst_build_kernel<16, 8, true>, 16);
        else if (stage == 16 && unroll == 16) go(fst_build_kernel<16, 16, true>, 16);
        else if (stage == 16 && unroll == 2) go(fst_build_kernel<16, 2, true>, 16);
        else if (stage == 8 && unroll == 8) go(fst_build_kernel<8, 8, true>, 8);
        else if (stage == 8 && unroll == 2) go(fst_build_kernel<8, 2, true>, 8);
        else if (stage == 4 && unroll == 2) go(fst_build_kernel<4, 2, true>, 4);
        else if (stage == 4) go(fst_build_kernel<4, 4, true>, 4);
        else if (stage == 8) go(fst_build_kernel<8, 4, true>, 8);
        else if (stage == 32) go(fst_build_kernel<32, 4, true>, 32);
        else go(fst_build_kernel<16, 4, true>, 16);
        return true;
    }
    return false;
}
