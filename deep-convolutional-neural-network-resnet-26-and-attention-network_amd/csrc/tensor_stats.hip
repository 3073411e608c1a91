// Per-tensor summaries of the tensors the other kernels left in HBM, read where they lie: channel-padded
// NHWC activations (fp32 or bf16, pad channels skipped) and flat fp32 runs inside the parameter / gradient buckets.  Reference:
// the per-layer activation summary the driver primes before an epoch and the per-parameter weight mean / max it records after
// one (gbm/classify_combined.py:418, :484-485).  One call = TWO launches for a whole table of tensors:
//   tensor_stats_partial_kernel  blockIdx.y = job; the job's bytes are cut into CHUNKS of 256 KiB counted from its first element,
//                                one workgroup per chunk (a workgroup walks chunks blockIdx.x, + gridDim.x, ...) -> one partial record
//   tensor_stats_finish_kernel   one workgroup per job adds the job's partial records in chunk order -> 8 doubles
// Summation order.  Element e of a job (counted from x, pad channels included) belongs to 16-byte piece e / VEC (VEC = 4 fp32 or
// 8 bf16), piece p to chunk p / 16384 and inside it to thread p % 256; a thread adds its pieces in rising order and the
// elements of a piece in rising order into ONE fp64 accumulator per statistic; the 256 accumulators of a chunk meet in a
// fixed butterfly (lanes), then wave 0..3 in order; chunks are added in index order.  All of that is a function of
// (n_pix, c_pad, dtype): not of the pointer's alignment (a 16-byte-misaligned run takes the SAME pieces with element loads), not
// of the grid, not of the other jobs.  No atomics: bit-repeatable.
#include "common.cuh"

#define MIL_STATS_THREADS 256
#define MIL_STATS_CHUNK_BYTES (256 * 1024)
#define MIL_STATS_CHUNK_PIECES (MIL_STATS_CHUNK_BYTES / 16)                       // 16384 = 64 per thread
#define MIL_STATS_GRID_X 2048                                                     // 8 workgroups on each of 256 CUs
#define MIL_STATS_MAX_CHUNKS (1ll << 24)                                          // 4 TiB per tensor
#define MIL_STATS_FIN_RECS 512                                                    // partial records staged per round of the finish

struct StatsJob {
    const void* x;
    long long n_pix;
    long long n_elems;              // n_pix * c_pad
    long long n_chunks;             // ceil(n_elems * element size / MIL_STATS_CHUNK_BYTES)
    int c_real, c_pad, dtype, pad_;
};

// A partial record and a thread's running state.  Counts of one chunk fit an int (131072 elements at most).
struct StatsAcc {
    double s, q;
    float mn, mx;
    int nfin, nneg;
};

__device__ __forceinline__ void stats_elem(StatsAcc& a, float v, bool counts) {
    const bool fin = counts && (__builtin_bit_cast(unsigned, v) & 0x7f800000u) != 0x7f800000u;
    const double d = (double)(fin ? v : 0.f);          // exact; adding +0.0 changes no sum (the sums start at +0.0)
    a.s += d;
    a.q = __builtin_fma(d, d, a.q);                    // d * d is exact in fp64: one rounding per element
    a.mn = (fin && v < a.mn) ? v : a.mn;
    a.mx = (fin && v > a.mx) ? v : a.mx;
    a.nfin += fin ? 1 : 0;
    a.nneg += (fin && v < 0.f) ? 1 : 0;                // -0.0 < 0 is false
}

template <int DT> struct StatsVec;
template <> struct StatsVec<MIL_DT_F32> { static constexpr int VEC = 4, ESZ = 4; };
template <> struct StatsVec<MIL_DT_BF16> { static constexpr int VEC = 8, ESZ = 2; };

// The tensor pointers come out of the job table, so the compiler cannot tell that they are global: said here, the loads are
// global_load_* instead of flat_load_*.
typedef __attribute__((address_space(1))) const char* stats_gptr;
typedef unsigned stats_u32x4 __attribute__((ext_vector_type(4)));
#define MIL_STATS_G(T, p) (*(__attribute__((address_space(1))) const T*)(p))

template <int DT> __device__ __forceinline__ float stats_load1(stats_gptr x, long long e) {
    if constexpr (DT == MIL_DT_F32) return MIL_STATS_G(float, x + e * 4);
    else return __builtin_bit_cast(float, (unsigned)MIL_STATS_G(unsigned short, x + e * 2) << 16);
}
template <int DT> __device__ __forceinline__ void stats_unpack(const stats_u32x4 r, float (&v)[StatsVec<DT>::VEC]) {
    // the elements are copied out first: __builtin_bit_cast applied to a vector ELEMENT (r.y) reads element 0 (hipcc, ROCm 7.2)
    const unsigned w[4] = {r.x, r.y, r.z, r.w};
    if constexpr (DT == MIL_DT_F32) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = __builtin_bit_cast(float, w[k]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[2 * k] = __builtin_bit_cast(float, w[k] << 16);
            v[2 * k + 1] = __builtin_bit_cast(float, w[k] & 0xffff0000u);
        }
    }
}

// MODE 0: every element counts (c_real == c_pad: flat runs, 40- and 80-channel maps); 1: c_pad is a multiple of VEC, so a piece
// lies inside one record and starts at a channel that is a multiple of VEC; 2: any record length (one 32-bit modulo per element).
template <int DT, int MODE> __device__ __forceinline__ bool stats_counts(unsigned c0, int j, unsigned c_real, unsigned c_pad) {
    if constexpr (MODE == 0) return true;
    else if constexpr (MODE == 1) return c0 + j < c_real;
    else return (c0 + j) % c_pad < c_real;
}

// The chunk [e0, e1) of a job (e0 a multiple of the chunk's element count) -> this thread's share of it.
template <int DT, int MODE>
__device__ __forceinline__ void stats_chunk(StatsAcc& a, stats_gptr x, long long e0, long long e1, unsigned c_real,
                                            unsigned c_pad, bool aligned) {
    constexpr int VEC = StatsVec<DT>::VEC, ESZ = StatsVec<DT>::ESZ, T = MIL_STATS_THREADS;
    constexpr int ITERS = MIL_STATS_CHUNK_PIECES / T;
    long long e = e0 + (long long)threadIdx.x * VEC;                   // first element of this thread's piece
    unsigned c0 = 0, step = 0;
    if constexpr (MODE != 0) {
        c0 = (unsigned)((unsigned long long)e % c_pad);
        step = (unsigned)(T * VEC) % c_pad;
    }
    auto advance = [&](unsigned c) { c += step; return c >= c_pad ? c - c_pad : c; };
    if (aligned && e1 - e0 == (long long)MIL_STATS_CHUNK_PIECES * VEC) {
        // a whole chunk of an aligned tensor: 16-byte loads, four in flight per thread, no bound to check
        for (int it = 0; it < ITERS; it += 4) {
            stats_u32x4 r[4];
            unsigned c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                r[u] = MIL_STATS_G(stats_u32x4, x + (e + (long long)u * T * VEC) * ESZ);
                c[u] = c0;
                c0 = advance(c0);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float v[VEC];
                stats_unpack<DT>(r[u], v);
#pragma unroll
                for (int j = 0; j < VEC; ++j) stats_elem(a, v[j], stats_counts<DT, MODE>(c[u], j, c_real, c_pad));
            }
            e += 4ll * T * VEC;
        }
        return;
    }
    // the ragged last chunk of a job, and every chunk of a run that does not start on a 16-byte boundary: the same pieces
    // in the same order, by element loads where the piece is not whole or not aligned
    for (int it = 0; it < ITERS && e < e1; ++it) {
        float v[VEC];
        if (aligned && e + VEC <= e1) {
            stats_unpack<DT>(MIL_STATS_G(stats_u32x4, x + e * ESZ), v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) stats_elem(a, v[j], stats_counts<DT, MODE>(c0, j, c_real, c_pad));
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const bool in = e + j < e1;
                const float vj = in ? stats_load1<DT>(x, e + j) : 0.f;
                stats_elem(a, vj, in && stats_counts<DT, MODE>(c0, j, c_real, c_pad));
            }
        }
        c0 = advance(c0);
        e += (long long)T * VEC;
    }
}

__device__ __forceinline__ void stats_merge(StatsAcc& a, const StatsAcc& b) {
    a.s += b.s; a.q += b.q;
    a.mn = b.mn < a.mn ? b.mn : a.mn;
    a.mx = b.mx > a.mx ? b.mx : a.mx;
    a.nfin += b.nfin; a.nneg += b.nneg;
}

// Partial record of a chunk: 8 words of 8 bytes: [0] finite count (int64) [1] sum [2] sum of squares [3] min [4] max (fp64)
// [5] negative count (int64) [6] [7] zero.
__global__ __launch_bounds__(MIL_STATS_THREADS, 4) void tensor_stats_partial_kernel(const StatsJob* __restrict__ jobs,
                                                                                 unsigned long long* __restrict__ ws,
                                                                                 long long slot_stride) {
    __shared__ double red_d[2][MIL_STATS_THREADS / 64];
    __shared__ float red_f[2][MIL_STATS_THREADS / 64];
    __shared__ int red_i[2][MIL_STATS_THREADS / 64];
    MIL_POISON_STATIC(red_d); MIL_POISON_STATIC(red_f); MIL_POISON_STATIC(red_i);
    const StatsJob* jp = jobs + blockIdx.y;
    const long long n_chunks = jp->n_chunks;
    if ((long long)blockIdx.x >= n_chunks) return;
    const stats_gptr x = (stats_gptr)jp->x;
    const long long n_elems = jp->n_elems;
    const unsigned c_real = (unsigned)jp->c_real, c_pad = (unsigned)jp->c_pad;
    const int dtype = jp->dtype;
    const bool aligned = ((uintptr_t)x & 15) == 0;
    const long long chunk_elems = (long long)MIL_STATS_CHUNK_BYTES / (dtype == MIL_DT_BF16 ? 2 : 4);
    const int vec = dtype == MIL_DT_BF16 ? 8 : 4;
    const int mode = c_real == c_pad ? 0 : (c_pad % vec == 0 ? 1 : 2);
    unsigned long long* slots = ws + (size_t)blockIdx.y * (size_t)slot_stride * 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const long long e0 = chunk * chunk_elems;
        const long long e1 = e0 + chunk_elems < n_elems ? e0 + chunk_elems : n_elems;
        StatsAcc a = {0.0, 0.0, __builtin_inff(), -__builtin_inff(), 0, 0};
        if (dtype == MIL_DT_BF16) {
            if (mode == 0) stats_chunk<MIL_DT_BF16, 0>(a, x, e0, e1, c_real, c_pad, aligned);
            else if (mode == 1) stats_chunk<MIL_DT_BF16, 1>(a, x, e0, e1, c_real, c_pad, aligned);
            else stats_chunk<MIL_DT_BF16, 2>(a, x, e0, e1, c_real, c_pad, aligned);
        } else {
            if (mode == 0) stats_chunk<MIL_DT_F32, 0>(a, x, e0, e1, c_real, c_pad, aligned);
            else if (mode == 1) stats_chunk<MIL_DT_F32, 1>(a, x, e0, e1, c_real, c_pad, aligned);
            else stats_chunk<MIL_DT_F32, 2>(a, x, e0, e1, c_real, c_pad, aligned);
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {            // the same tree in every lane (a + b == b + a bit for bit)
            StatsAcc b;
            b.s = __shfl_xor(a.s, m); b.q = __shfl_xor(a.q, m);
            b.mn = __shfl_xor(a.mn, m); b.mx = __shfl_xor(a.mx, m);
            b.nfin = __shfl_xor(a.nfin, m); b.nneg = __shfl_xor(a.nneg, m);
            stats_merge(a, b);
        }
        if (lane == 0) {
            red_d[0][wave] = a.s; red_d[1][wave] = a.q;
            red_f[0][wave] = a.mn; red_f[1][wave] = a.mx;
            red_i[0][wave] = a.nfin; red_i[1][wave] = a.nneg;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            StatsAcc t = {red_d[0][0], red_d[1][0], red_f[0][0], red_f[1][0], red_i[0][0], red_i[1][0]};
#pragma unroll
            for (int w = 1; w < MIL_STATS_THREADS / 64; ++w) {
                const StatsAcc b = {red_d[0][w], red_d[1][w], red_f[0][w], red_f[1][w], red_i[0][w], red_i[1][w]};
                stats_merge(t, b);
            }
            unsigned long long* rec = slots + (size_t)chunk * 8;
            rec[0] = (unsigned long long)(long long)t.nfin;
            rec[1] = __builtin_bit_cast(unsigned long long, t.s);
            rec[2] = __builtin_bit_cast(unsigned long long, t.q);
            rec[3] = __builtin_bit_cast(unsigned long long, (double)t.mn);
            rec[4] = __builtin_bit_cast(unsigned long long, (double)t.mx);
            rec[5] = (unsigned long long)(long long)t.nneg;
            rec[6] = 0; rec[7] = 0;
        }
        __syncthreads();                               // the LDS words are written again by the next chunk
    }
}

// One workgroup per job: the job's n_chunks partial records in index order -> out[job][8].  The records are fetched 512 at a
// time by all 256 threads (one 8-byte word each, sixteen in flight) and staged in LDS; thread t < 6 then walks word t of every
// record in order.  Each of those threads runs all four combinations (integer add, fp64 add, min, max) and keeps the one its
// word wants: no divergence inside the walk.
__global__ __launch_bounds__(MIL_STATS_THREADS) void tensor_stats_finish_kernel(const StatsJob* __restrict__ jobs,
                                                                                const unsigned long long* __restrict__ ws,
                                                                                long long slot_stride, double* __restrict__ out) {
    __shared__ unsigned long long buf[MIL_STATS_FIN_RECS * 8];
    MIL_POISON_STATIC(buf);
    const StatsJob* jp = jobs + blockIdx.x;
    const long long n_chunks = jp->n_chunks;
    const double total = (double)(jp->n_pix * (long long)jp->c_real);
    const unsigned long long* slots = ws + (size_t)blockIdx.x * (size_t)slot_stride * 8;
    const int t = threadIdx.x;
    unsigned long long ai = 0;
    double ad = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
    for (long long base = 0; base < n_chunks; base += MIL_STATS_FIN_RECS) {
        const long long left = n_chunks - base;
        const int nrec = left < MIL_STATS_FIN_RECS ? (int)left : MIL_STATS_FIN_RECS;
        const unsigned long long* src = slots + (size_t)base * 8;
        constexpr int PER = MIL_STATS_FIN_RECS * 8 / MIL_STATS_THREADS;
        unsigned long long v[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int w = t + u * MIL_STATS_THREADS;
            v[u] = w < nrec * 8 ? src[w] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) buf[t + u * MIL_STATS_THREADS] = v[u];
        __syncthreads();
        if (t < 6) {
#pragma unroll 8
            for (int r = 0; r < nrec; ++r) {
                const unsigned long long w = buf[r * 8 + t];
                const double d = __builtin_bit_cast(double, w);
                ai += w;
                ad += d;
                mn = d < mn ? d : mn;
                mx = d > mx ? d : mx;
            }
        }
        __syncthreads();
    }
    double* o = out + (size_t)blockIdx.x * 8;
    if (t == 0) { o[0] = (double)(long long)ai; o[6] = total - (double)(long long)ai; o[7] = total; }   // every real element is finite or not
    if (t == 1 || t == 2) o[t] = ad;
    if (t == 3) o[3] = mn;
    if (t == 4) o[4] = mx;
    if (t == 5) o[5] = (double)(long long)ai;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static int stats_job_check(const StatsJob& j) {
    if (!j.x || j.c_real < 1 || j.c_real > j.c_pad || j.n_pix < 0) return MIL_ERR_ARG;
    if (j.dtype != MIL_DT_F32 && j.dtype != MIL_DT_BF16) return MIL_ERR_UNSUPPORTED;
    const long long esz = j.dtype == MIL_DT_BF16 ? 2 : 4;
    if (j.n_pix > (MIL_STATS_MAX_CHUNKS * MIL_STATS_CHUNK_BYTES / esz) / j.c_pad) return MIL_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(j.x) & (uintptr_t)(esz - 1)) return MIL_ERR_ARG;
    const long long n_elems = j.n_pix * j.c_pad;
    const long long n_chunks = (n_elems * esz + MIL_STATS_CHUNK_BYTES - 1) / MIL_STATS_CHUNK_BYTES;
    if (j.n_elems != n_elems || j.n_chunks != n_chunks) return MIL_ERR_ARG;      // not a record mil_stats_job_fill wrote
    return MIL_OK;
}

// largest chunk count of the table = the slot pitch of the workspace (one 64-byte slot per chunk, [job][slot])
static int stats_table_check(const void* jobs_host, int njobs, long long* max_chunks) {
    const StatsJob* jobs = reinterpret_cast<const StatsJob*>(jobs_host);
    long long m = 0;
    for (int i = 0; i < njobs; ++i) {
        const int rc = stats_job_check(jobs[i]);
        if (rc != MIL_OK) return rc;
        if (jobs[i].n_chunks > m) m = jobs[i].n_chunks;
    }
    *max_chunks = m;
    return MIL_OK;
}

extern "C" int mil_stats_job_bytes(void) { return (int)sizeof(StatsJob); }

extern "C" int mil_stats_job_fill(void* job_host, const void* x, long long n_pix, int c_real, int c_pad, int dtype) {
    if (!job_host || !x || c_real < 1 || c_real > c_pad || n_pix < 0) return MIL_ERR_ARG;
    if (dtype != MIL_DT_F32 && dtype != MIL_DT_BF16) return MIL_ERR_UNSUPPORTED;
    const long long esz = dtype == MIL_DT_BF16 ? 2 : 4;
    if (n_pix > (MIL_STATS_MAX_CHUNKS * MIL_STATS_CHUNK_BYTES / esz) / c_pad) return MIL_ERR_ARG;
    StatsJob* j = reinterpret_cast<StatsJob*>(job_host);
    *j = StatsJob{};
    j->x = x; j->n_pix = n_pix; j->c_real = c_real; j->c_pad = c_pad; j->dtype = dtype;
    j->n_elems = n_pix * c_pad;
    j->n_chunks = (j->n_elems * esz + MIL_STATS_CHUNK_BYTES - 1) / MIL_STATS_CHUNK_BYTES;
    return stats_job_check(*j);
}

extern "C" int mil_tensor_stats_workspace(size_t* bytes, const void* jobs_host, int njobs) {
    if (!bytes || njobs < 0 || (njobs > 0 && !jobs_host)) return MIL_ERR_ARG;
    long long max_chunks = 0;
    const int rc = stats_table_check(jobs_host, njobs, &max_chunks);
    if (rc != MIL_OK) return rc;
    *bytes = (size_t)njobs * (size_t)(max_chunks > 0 ? max_chunks : 1) * 64;
    return MIL_OK;
}

extern "C" int mil_tensor_stats_all(const void* jobs_device, const void* jobs_host, int njobs, double* out, void* ws,
                                    size_t ws_bytes, void* stream) {
    if (njobs < 0) return MIL_ERR_ARG;
    if (njobs == 0) return MIL_OK;
    if (!jobs_device || !jobs_host || !out || !ws || njobs > 65535) return MIL_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(jobs_device)) & 7) return MIL_ERR_ARG;
    long long max_chunks = 0;
    const int rc = stats_table_check(jobs_host, njobs, &max_chunks);
    if (rc != MIL_OK) return rc;
    const long long slot_stride = max_chunks > 0 ? max_chunks : 1;
    if (ws_bytes < (size_t)njobs * (size_t)slot_stride * 64) return MIL_ERR_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const StatsJob* jd = reinterpret_cast<const StatsJob*>(jobs_device);
    if (max_chunks > 0) {
        const unsigned gx = (unsigned)(max_chunks < MIL_STATS_GRID_X ? max_chunks : MIL_STATS_GRID_X);
        hipLaunchKernelGGL(tensor_stats_partial_kernel, dim3(gx, (unsigned)njobs), dim3(MIL_STATS_THREADS), 0, s, jd,
                           static_cast<unsigned long long*>(ws), slot_stride);
        MIL_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(tensor_stats_finish_kernel, dim3((unsigned)njobs), dim3(MIL_STATS_THREADS), 0, s, jd,
                       static_cast<const unsigned long long*>(ws), slot_stride, out);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}
