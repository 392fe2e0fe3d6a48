// Scene files: the row move between the five parameter tensors of a scene and the (N, F) float32 rows of a 3DGS PLY body
// (mojosplat_amd/sceneio.py holds the file layout and the definition, pack_ply_rows_torch / unpack_ply_rows_torch; nothing in
// the reference does this: it reads and writes no scene).  Two kernels, k_ply_pack and k_ply_unpack, one launch each, no
// atomics, no host wait, no workspace.
//
// A column table says, for every file column it names, which (tensor, float offset in that tensor's row) it stands for, or
// none: pack writes +0.0 into such a column, unpack does not read it.  The kernels MOVE BITS: every value is a uint32 from
// the load to the store and passes through no float operation (a signalling NaN keeps its payload, -0.0 its sign).
//
// A workgroup owns kRows (64) consecutive rows.  Its slice of every array -- the file rows and each of the five tensors -- is
// one contiguous span that starts on a multiple of 256 bytes from the array's base, so it is moved by coalesced 16-byte
// accesses whenever the base is 16-byte aligned (dwords otherwise, and for the last < 4 floats of the last workgroup).
//   STAGE  the spans of the side that is read go to LDS as they are stored (pack: the five tensors' spans one after the other;
//          unpack: the rows' span).
//   EMIT   every lane builds four consecutive floats of a span of the side that is written, each from the LDS word the
//          compact table names: element e of a span of rows `width` floats wide is row r = e / width, position o = e - r width,
//          and comes from lds[src0[o] + r * stride[o]] (pack: src0 = the tensor's LDS base + offset, stride = the tensor's
//          width, or a word of zeros and stride 0; unpack: src0 = the file column, stride = S), then stores 16 bytes.
// The compact table (kMaxColumns words, src0 | stride << 16) is the kernel argument; its entries are read from LDS.
// Every global element index is 64-bit (size_t): N * F passes 2^31 from 35 M rows at degree 3.  Within a workgroup an index
// is below 64 * 192 and stays 32-bit.
#include "ms_common.hpp"

namespace {

constexpr int kRows = MS_PLY_ROWS;                 // rows of a workgroup
constexpr int kThreads = 256;
constexpr int kMaxColumns = MS_PLY_MAX_COLUMNS;
constexpr int kTensors = MS_PLY_TENSORS;
static_assert(kRows % 4 == 0, "a workgroup's span of a tensor of any width starts on a multiple of 16 bytes");
static_assert(kRows * MS_PLY_MAX_STRIDE < (1 << 16) && MS_PLY_MAX_STRIDE < (1 << 16), "src0 and stride share a 32-bit word");

struct Table {                                     // a kernel argument, by value
    uint32_t e[kMaxColumns];                       // src0 | stride << 16
};
struct Tensors {
    uint32_t *base[kTensors];
    uint32_t width[kTensors];
};
static_assert(sizeof(Table) == 512, "the table is a kernel argument: keep it small");

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// global span -> LDS, as stored.  lds is 16-byte aligned.
__device__ __forceinline__ void stage(const uint32_t *__restrict__ src, uint32_t count, uint32_t *lds) {
    const uint32_t tid = threadIdx.x;
    if (aligned16(src)) {
        const uint32_t n4 = count >> 2;
        for (uint32_t i = tid; i < n4; i += kThreads) ((uint4 *)lds)[i] = ((const uint4 *)src)[i];
        for (uint32_t i = (n4 << 2) + tid; i < count; i += kThreads) lds[i] = src[i];
    } else {
        for (uint32_t i = tid; i < count; i += kThreads) lds[i] = src[i];
    }
}

__device__ __forceinline__ uint32_t pick(const uint32_t *tab, const uint32_t *lds, uint32_t r, uint32_t o) {
    const uint32_t m = tab[o];
    return lds[(m & 0xFFFFu) + r * (m >> 16)];
}

// LDS -> global span of rows `width` floats wide, `count` floats; tab: the table's entries of this span's positions
__device__ __forceinline__ void emit(uint32_t *__restrict__ dst, uint32_t count, uint32_t width, const uint32_t *tab,
                                     const uint32_t *lds) {
    const uint32_t tid = threadIdx.x;
    uint32_t done = 0;
    if (aligned16(dst)) {
        const uint32_t n4 = count >> 2;
        for (uint32_t i = tid; i < n4; i += kThreads) {
            uint32_t r = (i << 2) / width, o = (i << 2) - r * width;
            uint32_t v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = pick(tab, lds, r, o);
                if (++o == width) o = 0, ++r;
            }
            ((uint4 *)dst)[i] = make_uint4(v[0], v[1], v[2], v[3]);
        }
        done = n4 << 2;
    }
    for (uint32_t e = done + tid; e < count; e += kThreads) {
        const uint32_t r = e / width;
        dst[e] = pick(tab, lds, r, e - r * width);
    }
}

// LDS: [kMaxColumns words of table][the staged spans][pack: 4 words of zeros]
extern __shared__ uint4 ply_lds4[];

__global__ void __launch_bounds__(kThreads)
k_ply_pack(const Table tab, const Tensors t, int64_t N, uint32_t F, uint32_t *__restrict__ rows) {
    uint32_t *s_tab = (uint32_t *)ply_lds4, *lds = s_tab + kMaxColumns;
    const int64_t row0 = (int64_t)blockIdx.x * kRows;
    const uint32_t n = (uint32_t)(N - row0 < kRows ? N - row0 : kRows);
    if (threadIdx.x < kMaxColumns) s_tab[threadIdx.x] = tab.e[threadIdx.x];
    uint32_t base = 0;
#pragma unroll
    for (int k = 0; k < kTensors; ++k) {
        stage(t.base[k] + (size_t)row0 * t.width[k], n * t.width[k], lds + base);
        base += kRows * t.width[k];
    }
    if (threadIdx.x < 4) lds[base + threadIdx.x] = 0u;              // what a column of no tensor reads
    __syncthreads();
    emit(rows + (size_t)row0 * F, n * F, F, s_tab, lds);
}

__global__ void __launch_bounds__(kThreads)
k_ply_unpack(const Table tab, const Tensors t, int64_t N, uint32_t S, const uint32_t *__restrict__ rows) {
    uint32_t *s_tab = (uint32_t *)ply_lds4, *lds = s_tab + kMaxColumns;
    const int64_t row0 = (int64_t)blockIdx.x * kRows;
    const uint32_t n = (uint32_t)(N - row0 < kRows ? N - row0 : kRows);
    if (threadIdx.x < kMaxColumns) s_tab[threadIdx.x] = tab.e[threadIdx.x];
    stage(rows + (size_t)row0 * S, n * S, lds);
    __syncthreads();
    uint32_t first = 0;                                              // the table holds the tensors' positions one after the other
#pragma unroll
    for (int k = 0; k < kTensors; ++k) {
        emit(t.base[k] + (size_t)row0 * t.width[k], n * t.width[k], t.width[k], s_tab + first, lds);
        first += t.width[k];
    }
}

// the checks both entry points share; sum_w: the five widths' sum
int check_common(const char *who, int64_t N, int F, const void *const *tensors, const int32_t *widths,
                 const ms_ply_column *columns, const void *rows, int *sum_w) {
    MS_REQUIRE(F >= 1 && F <= kMaxColumns, MS_ERR_INVALID_ARG, "%s: F = %d columns, not in [1, %d]", who, F, kMaxColumns);
    MS_REQUIRE(tensors && widths && columns && rows, MS_ERR_INVALID_ARG,
               "%s: null pointer (tensors, widths, columns or rows)", who);
    int sum = 0;
    for (int k = 0; k < kTensors; ++k) {
        MS_REQUIRE(tensors[k], MS_ERR_INVALID_ARG, "%s: null pointer (tensor %d)", who, k);
        MS_REQUIRE(((uintptr_t)tensors[k] & 3) == 0, MS_ERR_INVALID_ARG, "%s: misaligned pointer (tensor %d: float, 4 bytes)", who, k);
        MS_REQUIRE(widths[k] >= 1 && widths[k] <= kMaxColumns, MS_ERR_INVALID_ARG, "%s: tensor %d is %d floats wide, not in [1, %d]",
                   who, k, widths[k], kMaxColumns);
        sum += widths[k];
    }
    MS_REQUIRE(sum <= kMaxColumns, MS_ERR_INVALID_ARG, "%s: the tensors' rows hold %d floats together, more than %d", who, sum,
               kMaxColumns);
    MS_REQUIRE(((uintptr_t)rows & 3) == 0, MS_ERR_INVALID_ARG, "%s: misaligned pointer (rows: float, 4 bytes)", who);
    MS_REQUIRE(ms::ceil_div(N, kRows) <= 0x7FFFFFFF, MS_ERR_TOO_LARGE, "%s: %lld rows, more than a launch has workgroups for", who,
               (long long)N);
    for (int c = 0; c < F; ++c) {
        const ms_ply_column &e = columns[c];
        if (e.tensor == MS_PLY_NONE) continue;
        MS_REQUIRE(e.tensor >= 0 && e.tensor < kTensors, MS_ERR_INVALID_ARG, "%s: table entry %d names tensor %d, not in [0, %d)",
                   who, c, e.tensor, kTensors);
        MS_REQUIRE(e.offset >= 0 && e.offset < widths[e.tensor], MS_ERR_INVALID_ARG,
                   "%s: table entry %d has offset %d, outside its tensor's row width %d", who, c, e.offset, widths[e.tensor]);
    }
    *sum_w = sum;
    return MS_OK;
}

void fill(Tensors *t, const void *const *tensors, const int32_t *widths) {
    for (int k = 0; k < kTensors; ++k) {
        t->base[k] = (uint32_t *)tensors[k];
        t->width[k] = (uint32_t)widths[k];
    }
}

}  // namespace

extern "C" int ms_ply_pack(int64_t N, int F, const float *const *tensors, const int32_t *widths, const ms_ply_column *columns,
                           float *rows, void *stream) {
    MS_REQUIRE(N >= 0, MS_ERR_INVALID_ARG, "ply_pack: N < 0");
    if (N == 0) return MS_OK;
    int sum_w = 0;
    if (int rc = check_common("ply_pack", N, F, (const void *const *)tensors, widths, columns, rows, &sum_w)) return rc;
    uint32_t lds_base[kTensors], base = 0;
    for (int k = 0; k < kTensors; ++k) lds_base[k] = base, base += (uint32_t)(kRows * widths[k]);
    Table tab = {};
    bool seen[kMaxColumns] = {};
    for (int c = 0; c < F; ++c) {                      // every column of the rows is written, once
        const ms_ply_column &e = columns[c];
        MS_REQUIRE(e.column >= 0 && e.column < F, MS_ERR_INVALID_ARG, "ply_pack: table entry %d names column %d, not in [0, %d)", c,
                   e.column, F);
        MS_REQUIRE(!seen[e.column], MS_ERR_INVALID_ARG, "ply_pack: column %d is named twice", e.column);
        seen[e.column] = true;
        tab.e[e.column] = e.tensor == MS_PLY_NONE ? base                                     // the zeros, stride 0
                                                  : (lds_base[e.tensor] + (uint32_t)e.offset) | ((uint32_t)widths[e.tensor] << 16);
    }
    Tensors t;
    fill(&t, (const void *const *)tensors, widths);
    const size_t lds_bytes = (size_t)(kMaxColumns + kRows * sum_w + 4) * 4;
    hipLaunchKernelGGL(k_ply_pack, dim3((uint32_t)ms::ceil_div(N, kRows)), dim3(kThreads), lds_bytes, (hipStream_t)stream, tab, t, N,
                       (uint32_t)F, (uint32_t *)rows);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

extern "C" int ms_ply_unpack(int64_t N, int F, int S, const float *rows, float *const *tensors, const int32_t *widths,
                             const ms_ply_column *columns, void *stream) {
    MS_REQUIRE(N >= 0, MS_ERR_INVALID_ARG, "ply_unpack: N < 0");
    if (N == 0) return MS_OK;
    int sum_w = 0;
    if (int rc = check_common("ply_unpack", N, F, (const void *const *)tensors, widths, columns, rows, &sum_w)) return rc;
    MS_REQUIRE(S >= F && S <= MS_PLY_MAX_STRIDE, MS_ERR_INVALID_ARG, "ply_unpack: S = %d floats per row, not in [F = %d, %d]", S, F,
               MS_PLY_MAX_STRIDE);
    uint32_t first[kTensors], pos = 0;
    for (int k = 0; k < kTensors; ++k) first[k] = pos, pos += (uint32_t)widths[k];
    Table tab = {};
    bool seen[kMaxColumns] = {};
    int named = 0;
    for (int c = 0; c < F; ++c) {                      // every float of every tensor is written, once
        const ms_ply_column &e = columns[c];
        MS_REQUIRE(e.column >= 0 && e.column < S, MS_ERR_INVALID_ARG, "ply_unpack: table entry %d names column %d, not in [0, %d)", c,
                   e.column, S);
        if (e.tensor == MS_PLY_NONE) continue;
        const uint32_t p = first[e.tensor] + (uint32_t)e.offset;
        MS_REQUIRE(!seen[p], MS_ERR_INVALID_ARG, "ply_unpack: offset %d of tensor %d is named twice", e.offset, e.tensor);
        seen[p] = true, ++named;
        tab.e[p] = (uint32_t)e.column | ((uint32_t)S << 16);
    }
    MS_REQUIRE(named == sum_w, MS_ERR_INVALID_ARG, "ply_unpack: the table names %d of the tensors' %d floats per row (every one needs a column)",
               named, sum_w);
    Tensors t;
    fill(&t, (const void *const *)tensors, widths);
    const size_t lds_bytes = (size_t)(kMaxColumns + kRows * S) * 4;
    hipLaunchKernelGGL(k_ply_unpack, dim3((uint32_t)ms::ceil_div(N, kRows)), dim3(kThreads), lds_bytes, (hipStream_t)stream, tab, t, N,
                       (uint32_t)S, (const uint32_t *)rows);
    MS_LAUNCH_CHECK();
    return MS_OK;
}
