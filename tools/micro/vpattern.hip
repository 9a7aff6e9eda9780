// vpattern.hip -- what bounds the column pass's data movement? (round 3)
//
// The column pass (csrc/fgs_wave_v.hip) moves exactly its algorithmic bytes, yet runs at 4.6 TB/s where the row pass
// reaches 5.5: with the solve arithmetic removed it is no faster, so the limit is how the bytes move.  Its loads are
// "fragment-shaped": a thread owns (chunk, column pair), so one wave instruction fetches 8 rows x 64 bytes, 8 bytes per
// lane.  This program moves the same bytes of the same layout (strip-major weights, pair plane in 2-row tiles) with
//   L0  the kernel's own loads (8 B per lane, 8 half lines per instruction)
//   L1  LDS-DMA loads of whole 128-byte lines (16 B per lane, 8 lines per instruction) into a per-wave LDS ring, then
//       8-byte LDS reads into the same registers
//   S0  the kernel's own stores (8 B per lane)
//   S1  stores of whole lines (16 B per lane) staged through a per-wave LDS slot
// and prints the rate of every combination plus load-only / store-only legs.
//   hipcc -O3 --offload-arch=gfx950 tools/micro/vpattern.hip -o tools/micro/vpattern && tools/micro/vpattern [pairs]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

#ifndef VCW
#define VCW 16
#endif
#ifndef VTW
#define VTW 512
#endif
#ifndef NSLOTS
#define NSLOTS 12
#endif
constexpr int M = 34, VC = VCW, VT = VTW, TR = 2, NS = NSLOTS;   // VCW 8 + VTW 256: two independent half-width strips per CU
constexpr int XP = VC / 2, CH = VT / XP, LPR = VC / 2;   // column pairs, chunks per workgroup, 16-byte pieces per pair-plane row
constexpr int CPW = 64 / LPR;                            // chunks per wave instruction of the LDS-DMA
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

struct Args { float* C; float* U; int pitch, h; size_t plane; int delay; short* out; int out_w, out_x0; float* I; size_t image; };   // I: the last hand-off's register image, `image` floats per pair

template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }
__device__ __forceinline__ void wait_lds() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// one LDS-DMA instruction: every lane 16 bytes from its own address, image lane-linear at lds_dst (wave-uniform)
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

enum { F_GLDS = 1, F_LSTORE = 2, F_NOLOAD = 4, F_NOSTORE = 8, F_WINDOW = 16, F_PERSIST = 32,
       F_S16 = 64,      // stores as the LAST pass makes them: int16 row-major, 4 bytes per thread and row = a 32-byte piece per strip row
       F_S16T = 128,    // int16 into a tiled scratch [4-row tile][strip][4 rows][16 columns]: a strip's 4 rows are one whole 128-byte line
       F_REMAP = 256,   // strips b, b+8, b+16, b+24 (same XCD) on four adjacent strips, as the kernel's last pass   // F_WINDOW: L0 in groups of 8 rows, a wait per group
       F_IMG = 512 };   // right-hand sides from the last hand-off's register image [strip][wave][row in chunk][lane][U0 c0, U0 c1, U1 c0, U1 c1]:
                        // one 16-byte load per row, 1 KiB per wave instruction, 1 KiB from row to row (L0 form, whole strips)

struct Ctx {
    const char* bC; char* b0; unsigned tile_b, strip, h, rbase; int wv, lane, j, p, xp, cidx, r0;
};

// byte offset of pair-plane row `row` of the strip (start of its 128-byte line [U0 x16 | U1 x16])
__device__ __forceinline__ unsigned line_off(const Ctx& c, unsigned row, unsigned pitch)
{
    return ((row / TR) * (2u * TR * pitch) + c.strip * (2u * VC * TR) + (row % TR) * 2u * VC) * 4u;
}

template <int K, int MODE>
struct Items {
    // item K of the 51-item load sequence L0 L1 W0 L2 L3 W1 ...: K % 3 == 2 -> weight rows 2*(K/3), 2*(K/3)+1
    static __device__ __forceinline__ void issue(const Ctx& c, unsigned pitch, unsigned ring)
    {
        if constexpr (K < 51) {
            const unsigned slot = ring + (unsigned)(K % NS) * 1024u;
            if constexpr (K % 3 == 2) {
                const unsigned i2 = K / 3;
                constexpr int WP = VC / 4;                              // 16-byte pieces per weight row
                unsigned row = (unsigned)c.r0 + 2u * i2 + (unsigned)(c.p / WP);
                row = row < c.h ? row : c.rbase;
                glds16(c.bC + ((c.strip * c.h + row) * VC) * 4u + (unsigned)(c.p % WP) * 16u, slot);
            } else {
                const unsigned i = K - K / 3;
                unsigned row = (unsigned)c.r0 + i;
                row = row < c.h ? row : c.rbase;
                glds16(c.b0 + line_off(c, row, pitch) + (unsigned)c.p * 16u, slot);
            }
        }
    }
    static __device__ __forceinline__ void consume(const Ctx& c, const char* ringp, v2f (&cc)[M], v2f (&f0)[M], v2f (&f1)[M])
    {
        const char* s = ringp + (K % NS) * 1024 + c.j * (8 * VC) + c.xp * 8;
        if constexpr (K % 3 == 2) {
            cc[2 * (K / 3)] = *reinterpret_cast<const v2f*>(s);
            cc[2 * (K / 3) + 1] = *reinterpret_cast<const v2f*>(s + 4 * VC);
        } else {
            f0[K - K / 3] = *reinterpret_cast<const v2f*>(s);
            f1[K - K / 3] = *reinterpret_cast<const v2f*>(s + 4 * VC);
        }
    }
};

template <int K, int MODE>
__device__ __forceinline__ void glds_loop(const Ctx& c, unsigned pitch, unsigned ring, const char* ringp, v2f (&cc)[M], v2f (&f0)[M], v2f (&f1)[M])
{
    if constexpr (K < 51) {
        // items K .. min(K+NS-1, 50) are in flight: item K is done when at most that many minus one are outstanding
        constexpr int younger = (K + NS - 1 < 51 ? NS - 1 : 50 - K);
        wait_vm<younger>();
        Items<K, MODE>::consume(c, ringp, cc, f0, f1);
        wait_lds();                                          // the slot is free again
        Items<K + NS, MODE>::issue(c, pitch, ring);
        glds_loop<K + 1, MODE>(c, pitch, ring, ringp, cc, f0, f1);
    }
}

template <int K, int MODE>
__device__ __forceinline__ void glds_prime(const Ctx& c, unsigned pitch, unsigned ring)
{
    if constexpr (K < NS) { Items<K, MODE>::issue(c, pitch, ring); glds_prime<K + 1, MODE>(c, pitch, ring); }
}

template <int MODE>
__global__ void __launch_bounds__(VT, 2) vpat(Args a)
{
    extern __shared__ __align__(16) char lds[];
    const int tid = threadIdx.x;
    Ctx c;
    c.wv = tid >> 6; c.lane = tid & 63; c.j = c.lane / LPR; c.p = c.lane % LPR; c.xp = tid % XP; c.cidx = tid / XP;
    c.rbase = blockIdx.z * (CH * M); c.r0 = (int)c.rbase + c.cidx * M;     // blockIdx.z: which part of the column
    c.strip = blockIdx.x; c.h = (unsigned)a.h;
    if (MODE & F_REMAP) {
        const int nfull = (int)(gridDim.x / 32) * 32;
        if ((int)blockIdx.x < nfull) { const int grp = blockIdx.x >> 5, w = blockIdx.x & 31; c.strip = (unsigned)((grp << 5) + ((w & 7) << 2) + (w >> 3)); }
    }
    const size_t pb = (size_t)blockIdx.y * a.plane;
    c.bC = reinterpret_cast<const char*>(a.C + pb);
    c.b0 = reinterpret_cast<char*>(a.U + 2 * pb);
    const unsigned pitch = (unsigned)a.pitch;
    char* ringp = lds + c.wv * (NS * 1024);
    const unsigned ring = __builtin_amdgcn_readfirstlane((unsigned)(size_t)ringp);   // LDS byte address (wave-uniform -> SGPR)
    v2f cc[M], f0[M], f1[M];
#pragma unroll
    for (int i = 0; i < M; i++) { cc[i] = (v2f){1.f, 1.f}; f0[i] = (v2f){(float)i, 2.f}; f1[i] = (v2f){3.f, (float)tid}; }
    if (!(MODE & F_NOLOAD)) {
        if (MODE & F_GLDS) {
            glds_prime<0, MODE>(c, pitch, ring);
            glds_loop<0, MODE>(c, pitch, ring, ringp, cc, f0, f1);
        } else {
            // offsets walk down the rows as in the kernel (a 64-bit address or a division per row would cost registers)
            unsigned vo = line_off(c, (unsigned)c.r0, pitch) + c.xp * 8u, co = ((c.strip * c.h + (unsigned)c.r0) * VC + 2u * c.xp) * 4u;
            const unsigned vsafe = line_off(c, c.rbase, pitch) + c.xp * 8u, csafe = ((c.strip * c.h + c.rbase) * VC + 2u * c.xp) * 4u;
            const unsigned tile_b = 2u * TR * pitch * 4u;
            // (F_IMG: whole strips of 64 chunks only; rows past the column's end come from the image's own padding)
            const char* bI = reinterpret_cast<const char*>(a.I + (size_t)blockIdx.y * a.image);
            unsigned io = ((c.strip * (unsigned)(CH / 8) + (unsigned)c.wv) * (unsigned)M) * 1024u + (unsigned)c.lane * 16u;
#pragma unroll
            for (int i = 0; i < M; i++) {
                const bool ok = (unsigned)c.r0 + i < c.h;
                const unsigned v = ok ? vo : vsafe;
                cc[i] = *reinterpret_cast<const v2f*>(c.bC + (ok ? co : csafe));
                if constexpr ((MODE & F_IMG) != 0) {
                    const v4f q = *reinterpret_cast<const v4f*>(bI + io);
                    f0[i] = (v2f){q.x, q.y}; f1[i] = (v2f){q.z, q.w};
                    io += 1024u;
                } else {
                f0[i] = *reinterpret_cast<const v2f*>(c.b0 + v);
                f1[i] = *reinterpret_cast<const v2f*>(c.b0 + v + 4u * VC);
                }
                vo += ((((unsigned)c.r0 + i + 1u) & (TR - 1u)) == 0u) ? tile_b - (TR - 1u) * (8u * VC) : 8u * VC;
                co += 4u * VC;
                __builtin_amdgcn_sched_barrier(0);
                if ((MODE & F_WINDOW) && (i & 7) == 7) {
#pragma unroll
                    for (int k = i - 7; k <= i; k++) asm volatile("" : "+v"(cc[k]), "+v"(f0[k]), "+v"(f1[k]));
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < M; i++) { f0[i] = f0[i] * cc[i] + f1[i]; f1[i] = f1[i] - cc[i]; asm volatile("" : "+v"(f0[i]), "+v"(f1[i])); }
    if (a.delay > 0) {   // stands in for the solve: the whole workgroup meets, nothing moves for delay x 0.64 us (s_sleep 127 = 8128 clocks... measured)
        __syncthreads();
        for (int k = 0; k < a.delay; k++) __builtin_amdgcn_s_sleep(127);
        __syncthreads();
    }
    if (!(MODE & F_NOSTORE) && (MODE & (F_S16 | F_S16T))) {
        char* ob = reinterpret_cast<char*>(a.out + (size_t)blockIdx.y * ((size_t)a.out_w * a.h));
        const unsigned nstrips = (unsigned)a.pitch / VC;
        unsigned r0s = (unsigned)c.r0;
        asm volatile("" : "+v"(r0s));   // (the store phase's row arithmetic must not be shared with the load phase's)
        unsigned o = (MODE & F_S16T) ? ((r0s >> 2) * nstrips + c.strip) * (8u * VC) + (r0s & 3u) * (2u * VC) + 4u * c.xp
                                     : (r0s * (unsigned)a.out_w + (unsigned)a.out_x0 + c.strip * VC + 2u * c.xp) * 2u;
        asm volatile("" : "+v"(o));
#pragma unroll
        for (int i = 0; i < M; i++) {
            const unsigned row = r0s + i;
            if (row < c.h) {
                const float q0 = f0[i].x * f1[i].x, q1 = f0[i].y * f1[i].y;
                const unsigned v = ((unsigned)(unsigned short)(short)q0) | ((unsigned)(unsigned short)(short)q1 << 16);
                *reinterpret_cast<unsigned*>(ob + o) = v;
            }
            if (MODE & F_S16T) o += (((row + 1u) & 3u) == 0u) ? nstrips * (8u * VC) - 3u * (2u * VC) : 2u * VC;
            else o += 2u * (unsigned)a.out_w;
            __builtin_amdgcn_sched_barrier(0);
        }
    } else if (!(MODE & F_NOSTORE)) {
        if (MODE & F_LSTORE) {
            // per wave: rows i of its 8 chunks = 8 whole lines = one 1 KiB image, two slots alternating
            unsigned lo = line_off(c, (unsigned)c.r0, pitch) + (unsigned)c.p * 16u;   // (lane / LPR is the thread's own chunk)
            asm volatile("" : "+v"(lo));
            const unsigned tile_b2 = 2u * TR * pitch * 4u;
#pragma unroll
            for (int i = 0; i < M; i++) {
                char* s = ringp + (i & 3) * 1024;
                *reinterpret_cast<v2f*>(s + c.j * (8 * VC) + c.xp * 8) = f0[i];
                *reinterpret_cast<v2f*>(s + c.j * (8 * VC) + 4 * VC + c.xp * 8) = f1[i];
                wait_lds();
                const v4f q = *reinterpret_cast<const v4f*>(s + c.lane * 16);
                if ((unsigned)c.r0 + i < c.h) *reinterpret_cast<v4f*>(c.b0 + lo) = q;
                lo += ((((unsigned)c.r0 + i + 1u) & (TR - 1u)) == 0u) ? tile_b2 - (TR - 1u) * (8u * VC) : 8u * VC;
            }
        } else {
            unsigned vo = line_off(c, (unsigned)c.r0, pitch) + c.xp * 8u;
            asm volatile("" : "+v"(vo));
            const unsigned tile_b = 2u * TR * pitch * 4u;
#pragma unroll
            for (int i = 0; i < M; i++) {
                if ((unsigned)c.r0 + i < c.h) {
                    *reinterpret_cast<v2f*>(c.b0 + vo) = f0[i];
                    *reinterpret_cast<v2f*>(c.b0 + vo + 4u * VC) = f1[i];
                }
                vo += ((((unsigned)c.r0 + i + 1u) & (TR - 1u)) == 0u) ? tile_b - (TR - 1u) * (8u * VC) : 8u * VC;
            }
        }
    } else {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < M; i++) acc += f0[i].x + f0[i].y + f1[i].x + f1[i].y;
        if (acc == 123456.789f) a.U[0] = acc;                // keeps the loads alive
    }
}


// Persistent + software-pipelined: one workgroup per CU walks the strips of all pairs; the stores of strip k's row i are
// followed at once by the loads of row i of the NEXT strip into the same registers, so the CU never stops streaming
// (no store tail, no hand-over, no load ramp between strips).  delay: s_sleep(127) repetitions standing in for the solve.
template <int DELAY, bool S16 = false>
__global__ void __launch_bounds__(VT, 2) vpat_persist(Args a, int nstrips_total)
{
    const int tid = threadIdx.x;
    const unsigned xp = tid % XP, cidx = tid / XP, r0 = cidx * M, h = (unsigned)a.h, pitch = (unsigned)a.pitch;
    const int per_pair = a.pitch / VC;
    v2f cc[M], f0[M], f1[M];
    // wave-uniform bases of the current / next strip; per-thread row offsets are strip-independent
    auto base_u = [&](int s) { return reinterpret_cast<char*>(a.U + 2 * (size_t)(s / per_pair) * a.plane) + (size_t)(s % per_pair) * (2u * VC * TR) * 4u; };
    auto base_c = [&](int s) { return reinterpret_cast<const char*>(a.C + (size_t)(s / per_pair) * a.plane) + (size_t)(s % per_pair) * h * VC * 4u; };
    auto rowoff = [&](unsigned row) { return ((row / TR) * (2u * TR * pitch) + (row % TR) * 2u * VC) * 4u + xp * 8u; };
    // S16 (the last pass): four adjacent strips share the 128-byte lines of the int16 output, so they go to blocks with
    // equal blockIdx % 8 (one XCD under round-robin placement; speed only) in the same iteration
    const int bmap = S16 ? ((((int)blockIdx.x >> 5) * 8 + ((int)blockIdx.x & 7)) * 4 + (((int)blockIdx.x >> 3) & 3)) : (int)blockIdx.x;
    int s = (gridDim.x == 256u) ? bmap : (int)blockIdx.x;
    if (s >= nstrips_total) return;
    char* bu = base_u(s); const char* bc = base_c(s);
#pragma unroll
    for (int i = 0; i < M; i++) {
        unsigned row = r0 + i; row = row < h ? row : 0u;
        cc[i] = *reinterpret_cast<const v2f*>(bc + (row * VC + 2u * xp) * 4u);
        f0[i] = *reinterpret_cast<const v2f*>(bu + rowoff(row));
        f1[i] = *reinterpret_cast<const v2f*>(bu + rowoff(row) + 4u * VC);
        __builtin_amdgcn_sched_barrier(0);
    }
    while (true) {
#pragma unroll
        for (int i = 0; i < M; i++) { f0[i] = f0[i] * cc[i] + f1[i]; f1[i] = f1[i] - cc[i]; asm volatile("" : "+v"(f0[i]), "+v"(f1[i])); }
        __syncthreads();
        for (int k = 0; k < DELAY; k++) __builtin_amdgcn_s_sleep(127);
        __syncthreads();
        const int sn = s + gridDim.x;
        const bool more = sn < nstrips_total;
        char* bun = more ? base_u(sn) : bu; const char* bcn = more ? base_c(sn) : bc;
        unsigned ro = rowoff(r0), co = (r0 * VC + 2u * xp) * 4u;
        asm volatile("" : "+v"(ro), "+v"(co));
        const unsigned ro_safe = rowoff(0u), co_safe = (2u * xp) * 4u;
        const unsigned tile_b = 2u * TR * pitch * 4u;
        if (S16) {
            // results packed to int16 pairs first: the strip's 3 x M register pairs are free for the next strip's loads,
            // which are issued row by row in front of the (small) stores
            unsigned pk[M];
#pragma unroll
            for (int i = 0; i < M; i++) {
                const float q0 = f0[i].x * f1[i].x, q1 = f0[i].y * f1[i].y;
                pk[i] = ((unsigned)(unsigned short)(short)q0) | ((unsigned)(unsigned short)(short)q1 << 16);
            }
            char* ob = reinterpret_cast<char*>(a.out + (size_t)(s / per_pair) * ((size_t)a.out_w * a.h));
            unsigned oo = (r0 * (unsigned)a.out_w + (unsigned)a.out_x0 + (unsigned)(s % per_pair) * VC + 2u * xp) * 2u;
            if (!more) {                                     // last strip of this workgroup: stores only
#pragma unroll
                for (int i = 0; i < M; i++) {
                    if (r0 + i < h) *reinterpret_cast<unsigned*>(ob + oo) = pk[i];
                    oo += 2u * (unsigned)a.out_w;
                }
                break;
            }
#pragma unroll
            for (int i = 0; i < M; i++) {
                const bool ok = r0 + i < h;
                const unsigned r2 = ok ? ro : ro_safe;
                cc[i] = *reinterpret_cast<const v2f*>(bcn + (ok ? co : co_safe));
                f0[i] = *reinterpret_cast<const v2f*>(bun + r2);
                f1[i] = *reinterpret_cast<const v2f*>(bun + r2 + 4u * VC);
                if (ok) *reinterpret_cast<unsigned*>(ob + oo) = pk[i];
                ro += (((r0 + i + 1u) & (TR - 1u)) == 0u) ? tile_b - (TR - 1u) * (8u * VC) : 8u * VC;
                co += 4u * VC; oo += 2u * (unsigned)a.out_w;
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
        for (int i = 0; i < M; i++) {
            const bool ok = r0 + i < h;
            if (ok) {
                *reinterpret_cast<v2f*>(bu + ro) = f0[i];
                *reinterpret_cast<v2f*>(bu + ro + 4u * VC) = f1[i];
            }
            if (more) {                                      // (workgroup-uniform)
                const unsigned r2 = ok ? ro : ro_safe;
                cc[i] = *reinterpret_cast<const v2f*>(bcn + (ok ? co : co_safe));
                f0[i] = *reinterpret_cast<const v2f*>(bun + r2);
                f1[i] = *reinterpret_cast<const v2f*>(bun + r2 + 4u * VC);
            }
            ro += (((r0 + i + 1u) & (TR - 1u)) == 0u) ? tile_b - (TR - 1u) * (8u * VC) : 8u * VC;
            co += 4u * VC;
            __builtin_amdgcn_sched_barrier(0);
        }
        }
        if (!more) break;
        s = sn; bu = bun; bc = bcn;
    }
}

template <int DELAY, bool S16 = false>
float run_persist(const Args& a, int pairs, int reps, bool persistent)
{
    const int total = (a.pitch / VC) * pairs;
    dim3 grid(persistent ? 256 * (512 / VT) : total), block(VT);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int w = 0; w < 2; w++) hipLaunchKernelGGL((vpat_persist<DELAY, S16>), grid, block, 0, 0, a, total);
    CK(hipEventRecord(e0));
    for (int r = 0; r < reps; r++) hipLaunchKernelGGL((vpat_persist<DELAY, S16>), grid, block, 0, 0, a, total);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
    float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
    return ms / reps;
}

template <int MODE>
float run(const Args& a, int pairs, int reps, size_t lds)
{
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(vpat<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    dim3 grid(a.pitch / VC, pairs, (a.h + CH * M - 1) / (CH * M)), block(VT);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int w = 0; w < 2; w++) hipLaunchKernelGGL(vpat<MODE>, grid, block, lds, 0, a);
    CK(hipEventRecord(e0));
    for (int r = 0; r < reps; r++) hipLaunchKernelGGL(vpat<MODE>, grid, block, lds, 0, a);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
    float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
    return ms / reps;
}

// ---- the third row pass's side of the last hand-off ----
// One wavefront per image row of the 3584-column ROI (the M = 56 row bucket, 18 KiB of LDS per workgroup as the guide
// forms have: two waves per SIMD): the row's 28 float4s per lane are loaded from the pair plane exactly as the row pass
// loads them (128-byte pieces at a 256-byte stride) and stored
//   H_PAIR   back where they came from (the pair plane: eight 128-byte pieces at a 256-byte stride per instruction)
//   H_IMAGE  as whole 128-byte lines at the register image's addresses (eight lines per instruction, one per strip,
//            8 * M KiB apart; the lines of consecutive rows of a chunk are 1 KiB apart)
// H_NOLOAD / H_NOSTORE: one leg alone.
enum { H_PAIR = 0, H_IMAGE = 1, H_NOLOAD = 2, H_NOSTORE = 4 };
template <int HM>
__global__ void __launch_bounds__(64) hpat(Args a)
{
    constexpr int NV = 28;                                   // float4s per lane of a pair row of 3584 columns
    const unsigned lane = threadIdx.x, y = blockIdx.x, pitch = (unsigned)a.pitch, nvec = 2u * pitch / 4u;
    v4f* s = reinterpret_cast<v4f*>(a.U + 2 * (size_t)blockIdx.y * a.plane + (size_t)(y / TR) * (2u * TR * pitch) + (y % TR) * 32u);
    const unsigned chunk = y / (unsigned)M, i = y % (unsigned)M;
    v4f* d = reinterpret_cast<v4f*>(a.I + (size_t)blockIdx.y * a.image) + (chunk / 8u) * (unsigned)(M * 64) + i * 64u + (chunk % 8u) * 8u;
    v4f t[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) {
        const unsigned q = 64u * k + lane;
        t[k] = (v4f){(float)k, 1.f, 2.f, (float)lane};
        if (!(HM & H_NOLOAD) && q < nvec) t[k] = __builtin_nontemporal_load(s + (q >> 3) * (8u * TR) + (q & 7u));
    }
#pragma unroll
    for (int k = 0; k < NV; k++) asm volatile("" : "+v"(t[k]));
    if (HM & H_NOSTORE) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < NV; k++) acc += t[k].x + t[k].y + t[k].z + t[k].w;
        if (acc == 123456.789f) a.U[0] = acc;
        return;
    }
    unsigned lane_s = lane;
    asm volatile("" : "+v"(lane_s));                         // (the store addresses are formed after the loads, as in the row pass)
#pragma unroll
    for (int k = 0; k < NV; k++) {
        const unsigned q = 64u * k + lane_s;
        if (q < nvec) {
            if (HM & H_IMAGE) __builtin_nontemporal_store(t[k], d + (size_t)(q >> 3) * (unsigned)(512 * M) + (q & 7u));
            else __builtin_nontemporal_store(t[k], s + (q >> 3) * (8u * TR) + (q & 7u));
        }
    }
}

template <int HM>
float run_h(const Args& a, int pairs, int reps)
{
    const size_t lds = 18 * 1024;
    dim3 grid(a.h, pairs), block(64);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int w = 0; w < 2; w++) hipLaunchKernelGGL(hpat<HM>, grid, block, lds, 0, a);
    CK(hipEventRecord(e0));
    for (int r = 0; r < reps; r++) hipLaunchKernelGGL(hpat<HM>, grid, block, lds, 0, a);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
    float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
    return ms / reps;
}

// The last hand-off, both sides, pair plane against register image; `rounds` repetitions of the whole series so that
// the pair plane's own spread in this run is on the page.
static void handoff(Args a, int pairs, int rounds, size_t lds)
{
    printf("last hand-off, %d pairs of 3584 x 2160 (x64/pairs in ms): third row pass's pattern and last column pass's pattern\n", pairs);
    const double sc = 64.0 / pairs;
    for (int r = 0; r < rounds; r++) {
        const float hp = run_h<H_PAIR>(a, pairs, 10), hi = run_h<H_IMAGE>(a, pairs, 10);
        const float hl = run_h<H_NOSTORE>(a, pairs, 10), sp = run_h<H_PAIR | H_NOLOAD>(a, pairs, 10), si = run_h<H_IMAGE | H_NOLOAD>(a, pairs, 10);
        a.delay = 0;
        const float vp0 = run<F_S16 | F_REMAP>(a, pairs, 10, lds), vi0 = run<F_S16 | F_REMAP | F_IMG>(a, pairs, 10, lds);
        const float lp = run<F_NOSTORE | F_REMAP>(a, pairs, 10, lds), li = run<F_NOSTORE | F_REMAP | F_IMG>(a, pairs, 10, lds);
        a.delay = 2;
        const float vp2 = run<F_S16 | F_REMAP>(a, pairs, 10, lds), vi2 = run<F_S16 | F_REMAP | F_IMG>(a, pairs, 10, lds);
        a.delay = 0;
        printf("  round %d  row: load+store pair %.3f image %.3f | loads only %.3f | stores only pair %.3f image %.3f\n", r, hp * sc, hi * sc, hl * sc, sp * sc, si * sc);
        printf("  round %d  col: loads+int16 rows, no solve pair %.3f image %.3f | 7 us solve pair %.3f image %.3f | loads only pair %.3f image %.3f\n",
               r, vp0 * sc, vi0 * sc, vp2 * sc, vi2 * sc, lp * sc, li * sc);
        printf("  round %d  sum (row + col with 7 us solve): pair %.3f image %.3f  difference %+.3f\n", r, (hp + vp2) * sc, (hi + vi2) * sc, (hi + vi2 - hp - vp2) * sc);
    }
}

// An INNER hand-off's column side: the plain column pass (consecutive blocks on consecutive strips, 8-byte stores of
// both right-hand sides to the pair plane, the Cvert stream as it is) with its right-hand sides loaded from the pair
// plane as today against one 16-byte load per row from the register image.  `rounds` repetitions so that the pair
// plane's own spread in this run is on the page; the last line is the gate of the change that built the kernels.
static void inner_handoff(Args a, int pairs, int rounds, size_t lds)
{
    printf("inner hand-off, %d pairs of 3584 x 2160 (x64/pairs in ms): plain column pass's pattern, loads from pair plane | register image, stores to the pair plane\n", pairs);
    const double sc = 64.0 / pairs;
    float pmin = 1e30f, pmax = 0.f, imin = 1e30f, imax = 0.f;
    for (int r = 0; r < rounds; r++) {
        a.delay = 0;
        const float vp0 = run<0>(a, pairs, 10, lds), vi0 = run<F_IMG>(a, pairs, 10, lds);
        const float lp = run<F_NOSTORE>(a, pairs, 10, lds), li = run<F_NOSTORE | F_IMG>(a, pairs, 10, lds);
        a.delay = 2;
        const float vp2 = run<0>(a, pairs, 10, lds), vi2 = run<F_IMG>(a, pairs, 10, lds);
        a.delay = 0;
        pmin = vp2 < pmin ? vp2 : pmin; pmax = vp2 > pmax ? vp2 : pmax; imin = vi2 < imin ? vi2 : imin; imax = vi2 > imax ? vi2 : imax;
        printf("  round %d  col: loads+pair-plane stores, no solve pair %.3f image %.3f | 7 us solve pair %.3f image %.3f (%+.3f) | loads only pair %.3f image %.3f\n",
               r, vp0 * sc, vi0 * sc, vp2 * sc, vi2 * sc, (vi2 - vp2) * sc, lp * sc, li * sc);
    }
    printf("  with the 7 us solve: pair %.3f-%.3f (spread %.3f)  image %.3f-%.3f  smallest gap (pair min - image max) %+.3f  = %.1f x the pair plane's spread\n",
           pmin * sc, pmax * sc, (pmax - pmin) * sc, imin * sc, imax * sc, (pmin - imax) * sc, (pmin - imax) / (pmax - pmin > 0.f ? pmax - pmin : 1e-6f));
}

__global__ void fill_kernel(float* p, size_t n, unsigned seed)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = (float)((((unsigned)i + seed) * 2654435761u) >> 12) * (1.0f / 1048576.0f);
}

// L1+S1 and every mix must produce exactly what L0+S0 produces on the same data
static bool verify()
{
    Args a; a.pitch = 3584; a.h = 2160; a.plane = (size_t)a.pitch * a.h; a.delay = 0; a.out = nullptr; a.out_w = 3840; a.out_x0 = 256; a.I = nullptr; a.image = 0;
    float* U[4];
    CK(hipMalloc(&a.C, a.plane * 4));
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((a.plane + 255) / 256)), dim3(256), 0, 0, a.C, a.plane, 7u);
    const size_t lds = (VT / 64) * NS * 1024 + 44 * 1024 * VC / 16;
    std::vector<float> ref(a.plane * 2), got(a.plane * 2);
    bool ok = true;
    for (int m = 0; m < 4; m++) {
        CK(hipMalloc(&U[m], a.plane * 8));
        hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((a.plane * 2 + 255) / 256)), dim3(256), 0, 0, U[m], a.plane * 2, 99u);
        a.U = U[m];
        dim3 grid(a.pitch / VC, 1, (a.h + CH * M - 1) / (CH * M)), block(VT);
        if (m == 0) hipLaunchKernelGGL(vpat<0>, grid, block, lds, 0, a);
        if (m == 1) { CK(hipFuncSetAttribute(reinterpret_cast<const void*>(vpat<F_GLDS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); hipLaunchKernelGGL(vpat<F_GLDS>, grid, block, lds, 0, a); }
        if (m == 2) { CK(hipFuncSetAttribute(reinterpret_cast<const void*>(vpat<F_LSTORE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); hipLaunchKernelGGL(vpat<F_LSTORE>, grid, block, lds, 0, a); }
        if (m == 3) { CK(hipFuncSetAttribute(reinterpret_cast<const void*>(vpat<F_GLDS | F_LSTORE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); hipLaunchKernelGGL(vpat<F_GLDS | F_LSTORE>, grid, block, lds, 0, a); }
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(m == 0 ? ref.data() : got.data(), U[m], a.plane * 8, hipMemcpyDeviceToHost));
        if (m > 0) {
            size_t bad = 0;
            for (size_t i = 0; i < ref.size(); i++) bad += ref[i] != got[i];
            printf("  verify mode %d vs the kernel's own pattern: %zu differing floats\n", m, bad);
            ok = ok && bad == 0;
        }
        CK(hipFree(U[m]));
    }
    CK(hipFree(a.C));
    return ok;
}

int main(int argc, char** argv)
{
    if (!verify()) { printf("VERIFY FAILED\n"); return 1; }
    const int pairs = argc > 1 ? atoi(argv[1]) : 16;
    Args a; a.pitch = 3584; a.h = 2160; a.plane = (size_t)a.pitch * a.h; a.delay = 0;
    CK(hipMalloc(&a.C, a.plane * 4 * pairs)); CK(hipMalloc(&a.U, a.plane * 8 * pairs));
    a.out_w = 3840; a.out_x0 = 256; CK(hipMalloc(&a.out, (size_t)a.out_w * a.h * 2 * pairs));
    CK(hipMemset(a.C, 0, a.plane * 4 * pairs)); CK(hipMemset(a.U, 0, a.plane * 8 * pairs));
    a.image = (size_t)a.pitch * (CH * M) * 2;                 // every strip holds CH * M rows, the column's padding included
    CK(hipMalloc(&a.I, a.image * 4 * pairs)); CK(hipMemset(a.I, 0, a.image * 4 * pairs));
    const double px = (double)a.plane * pairs;
    const size_t lds = (VT / 64) * NS * 1024 + 44 * 1024 * VC / 16;   // the real kernel's exchange buffers ride along
    if (argc > 2 && VC == 16 && VT == 512) {                  // vpattern <pairs> <rounds>: the last hand-off's series only
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(vpat<F_S16 | F_REMAP | F_IMG>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (argc > 3 && argv[3][0] == 'i') inner_handoff(a, pairs, atoi(argv[2]), lds);   // vpattern <pairs> <rounds> inner
        else handoff(a, pairs, atoi(argv[2]), lds);
        return 0;
    }
    struct { const char* name; float ms; double bytes; } r[] = {
        {"L0+S0 (as the kernel)", run<0>(a, pairs, 10, lds), 20 * px},
        {"L1+S0 (LDS-DMA whole lines)", run<F_GLDS>(a, pairs, 10, lds), 20 * px},
        {"L0+S1 (whole-line stores)", run<F_LSTORE>(a, pairs, 10, lds), 20 * px},
        {"L1+S1", run<F_GLDS | F_LSTORE>(a, pairs, 10, lds), 20 * px},
        {"L0w+S0 (8-row windows)", run<F_WINDOW>(a, pairs, 10, lds), 20 * px},
        {"L0 only", run<F_NOSTORE>(a, pairs, 10, lds), 12 * px},
        {"L1 only", run<F_GLDS | F_NOSTORE>(a, pairs, 10, lds), 12 * px},
        {"S0 only", run<F_NOLOAD>(a, pairs, 10, lds), 8 * px},
        {"S1 only", run<F_NOLOAD | F_LSTORE>(a, pairs, 10, lds), 8 * px},
        {"L0+S16 (last pass: int16 rows)", run<F_S16>(a, pairs, 10, lds), 14 * px},
        {"L0+S16 remapped strips", run<F_S16 | F_REMAP>(a, pairs, 10, lds), 14 * px},
        {"L0+S16T (int16, tiled lines)", run<F_S16T>(a, pairs, 10, lds), 14 * px},
        {"S16 only", run<F_S16 | F_NOLOAD>(a, pairs, 10, lds), 2 * px},
        {"S16 only, remapped strips", run<F_S16 | F_REMAP | F_NOLOAD>(a, pairs, 10, lds), 2 * px},
        {"S16T only", run<F_S16T | F_NOLOAD>(a, pairs, 10, lds), 2 * px},
    };
    if (VC == 16 || VT == 256) {
        struct { const char* name; float ms; } q[] = {
            {"one workgroup per strip, no solve", run_persist<0>(a, pairs, 10, false)},
            {"one workgroup per strip, 7 us solve", run_persist<2>(a, pairs, 10, false)},
            {"persistent + pipelined, no solve", run_persist<0>(a, pairs, 10, true)},
            {"persistent + pipelined, 7 us solve", run_persist<2>(a, pairs, 10, true)},
        };
        a.delay = 2;
        const float l0 = run<F_S16 | F_REMAP>(a, pairs, 10, lds);
        a.delay = 0;
        struct { const char* name; float ms; } q16[] = {
            {"last pass (int16 rows): one workgroup per strip, 7 us solve", l0},
            {"last pass: persistent, next strip's loads before the stores, no solve", run_persist<0, true>(a, pairs, 10, true)},
            {"last pass: persistent, next strip's loads before the stores, 7 us solve", run_persist<2, true>(a, pairs, 10, true)},
        };
        for (auto& x : q16) printf("  %-72s %8.3f ms  (x64/pairs: %.3f ms)\n", x.name, x.ms, x.ms * 64.0 / pairs);
        for (auto& x : q) printf("  %-40s %8.3f ms  %7.1f GB/s  (x64/pairs: %.3f ms)\n", x.name, x.ms, 20 * px / x.ms / 1e6, x.ms * 64.0 / pairs);
    }
    printf("column-pass data movement, %d pairs of 3584 x 2160, strips of %d columns, %d chunks of %d rows per workgroup, %d workgroup(s) per strip\n", pairs, VC, CH, M, (a.h + CH * M - 1) / (CH * M));
    for (auto& x : r) printf("  %-32s %8.3f ms  %7.1f GB/s  (x64/pairs: %.3f ms)\n", x.name, x.ms, x.bytes / x.ms / 1e6, x.ms * 64.0 / pairs);
    // the same with a stand-in for the solve between loads and stores (workgroup barrier, s_sleep, barrier)
    for (int d = 1; d <= 8; d *= 2) {
        a.delay = d;
        const float t0 = run<0>(a, pairs, 10, lds), t1 = run<F_GLDS>(a, pairs, 10, lds);
        printf("  solve stand-in %d x s_sleep(127):  L0+S0 %8.3f ms (x64/pairs: %.3f ms)   L1+S0 %8.3f ms (x64/pairs: %.3f ms)\n", d, t0, t0 * 64.0 / pairs, t1, t1 * 64.0 / pairs);
    }
    return 0;
}
