// vs_ring.h -- the per-wave LDS tile ring of the 128-d scans (scan_kernel, scan_i8w_kernel, scan_f32s_kernel,
// scan_one_kernel): its layout, the LDS-DMA that fills it, and the operand loads and waits that the compiler does not
// see.  Device code only.
//
// A wave owns kRingDepth slots.  A slot is 8 KB of rows -- one 16-row tile of fp32 rows, or one 64-row tile of byte rows
// -- followed by 256 bytes of row terms (squared norms / int8 row terms of up to 64 rows).  It is filled by kRingPieces
// LDS-DMA instructions: piece j (0..7) writes LDS chunks [64 j, 64 j + 64) of the slot (a chunk is 16 bytes), piece 8
// the row terms.
//   fp32: lane l lands at row 2 j + (l >> 5), stored chunk (l & 31)  <-  source chunk (l & 31) ^ row
//   int8: 128-byte rows, piece j moves rows 8j..8j+7; lane l lands at row 8j + (l >> 3), stored chunk l & 7
//         <-  source chunk (l & 7) ^ ((row >> 1) & 7)
// The XOR is applied to the DMA *source* address, the LDS side stays lane-linear; it makes the ds_read_b128 of the A
// fragments conflict free.  The per-lane byte offsets inside a tile are fixed, so a DMA is "scalar tile base + 32-bit
// lane offset" with no address arithmetic in the loop: while the other wave of the SIMD streams MFMAs, every extra VALU
// instruction here costs about one MFMA slot.  Rows past the end are fetched unclamped (every row array has kScanPadRows
// spare rows) and masked where candidates are taken.
//
// The only VMEM operations of a tile loop are these pieces, and they are counted by hand: "s_waitcnt vmcnt(N)" stands
// where exactly N younger operations follow the data needed, N written in terms of kRingPieces.  Nothing drains the
// queue, and no barrier is needed because a wave reads only what it loaded itself.
#pragma once
#include "vs_kernels.h"
#include <utility>

namespace vs {

constexpr int kRingPieces = 9;                    // vector-memory instructions per tile: 8 row pieces + the row terms
constexpr int kRingTermOffset = kTileRows * kDim * 4;  // 8192: the row terms behind the rows
constexpr int kRingSlotBytes = kRingTermOffset + 256;
constexpr int kRingDepth = 2;
constexpr int kRingWaveBytes = kRingDepth * kRingSlotBytes;

// ---- offset tables ----
// voff[j]: this lane's byte offset inside a tile of the 16 bytes that piece j moves for it (layout above)
__device__ __forceinline__ void ring_src_offsets_f32(const int lane, unsigned (&voff)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int row_in = 2 * j + (lane >> 5);
        voff[j] = (unsigned)(row_in * 512 + 16 * ((lane & 31) ^ row_in));
    }
}
__device__ __forceinline__ void ring_src_offsets_i8(const int lane, unsigned (&voff)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int row_in = 8 * j + (lane >> 3);
        voff[j] = (unsigned)(row_in * 128 + 16 * ((lane & 7) ^ ((row_in >> 1) & 7)));
    }
}
// LDS byte offsets of lane (r, g)'s A fragments inside slot 0 of the ring that starts at byte wave_base (slot 1:
// + kRingSlotBytes, an immediate once the slot is a compile-time constant).  fp32: fa[c] = row r, chunk (4 c + g) ^ r;
// fa_n = the norms of rows 4 g .. 4 g + 3.
__device__ __forceinline__ void ring_frag_offsets_f32(const int wave_base, const int r, const int g, unsigned (&fa)[8], unsigned& fa_n) {
#pragma unroll
    for (int c = 0; c < 8; ++c) fa[c] = (unsigned)(wave_base + r * 512 + (((4 * c + g) ^ r) << 4));
    fa_n = (unsigned)(wave_base + kRingTermOffset + 16 * g);
}
// int8: c = 2 rg + half: row 16 rg + r, chunk (4 half + g) ^ ((row >> 1) & 7); fa_n = the row terms of rows 4 g .. 4 g + 3
// (+ 64 rg bytes for 16-row block rg)
__device__ __forceinline__ void ring_frag_offsets_i8(const int wave_base, const int r, const int g, unsigned (&fa)[8], unsigned& fa_n) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int row_in = 16 * (c >> 1) + r;
        fa[c] = (unsigned)(wave_base + row_in * 128 + ((((c & 1) * 4 + g) ^ ((row_in >> 1) & 7)) << 4));
    }
    fa_n = (unsigned)(wave_base + kRingTermOffset + 16 * g);
}

// ---- LDS-DMA written as instructions ----
// One piece: 16 bytes per lane from base + voff to LDS dst + OFF + 16 lane ("scalar base + this lane's 32-bit offset";
// no instruction offset: it would move the LDS address as well as the global one).  M0 = the LDS address, by one scalar
// add, one wait state ahead of the instruction that reads it.  (Through the builtin every piece cost two vector
// instructions -- a register copy and the M0 value read back from a spilled scalar -- and a vector instruction costs an
// MFMA-bound loop about 8 cycles of MFMA pipe.)  NT: the rows are streamed once and never fit a cache.
//
// M0 is written and read inside ONE statement, so nothing of the compiler's can fall between the write and the DMA;
// it is left changed behind the statement, without a declaration (an "m0" clobber is refused as a reserved register).
// That is sound because the compiler keeps no value in M0 across statements here: on gfx9 its LDS instructions do not
// read M0, and what does read it (an LDS-DMA builtin, s_movrel, a message) gets its M0 written directly in front.  The
// kernels that use these pieces contain no such instruction of the compiler's at all (their disassembly has no M0
// outside these statements); scan_kernel, which issues through the builtin, does not use them.  scan_f32f_kernel's
// unit issue saves and restores M0 around each piece instead, which needs no such argument: it pays two scalar moves
// for that on 2 kPieces + 1 pieces per 64 rows, where a tile ring issues kRingPieces per 16 rows in an MFMA-bound loop
// and folds the piece offset into the one scalar add.
template <int OFF, bool NT>
__device__ __forceinline__ void ring_dma_piece(const unsigned dst, const unsigned voff, const char* base) {
    if constexpr (NT) asm volatile("s_add_u32 m0, %0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt" ::"s"(dst), "v"(voff), "s"(base), "n"(OFF) : "memory", "scc");
    else asm volatile("s_add_u32 m0, %0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(dst), "v"(voff), "s"(base), "n"(OFF) : "memory", "scc");
}
// the row terms: one dword per lane (lane l <- term of row l), never nt
__device__ __forceinline__ void ring_dma_terms(const unsigned dst, const unsigned voff_n, const char* base) {
    asm volatile("s_add_u32 m0, %0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2" ::"s"(dst), "v"(voff_n), "s"(base), "n"(kRingTermOffset) : "memory", "scc");
}
// the eight 1 KB row pieces of a slot: piece j from base + voff[j] to dst + 1024 j
template <bool NT, int... J>
__device__ __forceinline__ void ring_dma_rows(const unsigned dst, const char* base, const unsigned (&voff)[8], std::integer_sequence<int, J...>) {
    (ring_dma_piece<J * 1024, NT>(dst, voff[J], base), ...);
}
template <bool NT>
__device__ __forceinline__ void ring_dma_rows(const unsigned dst, const char* base, const unsigned (&voff)[8]) {
    ring_dma_rows<NT>(dst, base, voff, std::make_integer_sequence<int, 8>{});
}
// a whole tile into the slot at LDS address dst (wave-uniform): kRingPieces instructions
template <bool NT>
__device__ __forceinline__ void ring_issue_tile(const unsigned dst, const char* tile_base, const char* term_base, const unsigned (&voff)[8], const unsigned voff_n) {
    ring_dma_rows<NT>(dst, tile_base, voff);
    ring_dma_terms(dst, voff_n, term_base);
}

// ---- operand loads the compiler does not see, and their waits ----
// A register load written as an instruction is no memory operation to the compiler: it puts no s_waitcnt of its own in
// front of the first use (that would be vmcnt(0), a drain of the tile queue).  The wait is wait_vm<N>() -- N = the
// vector-memory operations issued after the load -- and directly behind it every loaded register goes through
// tie_loaded(): the register becomes an in/out operand of an empty statement that cannot move above the wait, and
// whatever reads it afterwards depends on that statement by data flow.  Without the tie nothing but instruction order
// keeps a consumer (or a register copy the compiler makes) behind the wait; that was seen to break a test at random.
template <class V>
__device__ __forceinline__ void asm_load_b128(V& dst, const void* src) {
    static_assert(sizeof(V) == 16, "a four-dword register group");
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(src) : "memory");
}
template <class V>
__device__ __forceinline__ void asm_load_b32(V& dst, const void* src) {
    static_assert(sizeof(V) == 4, "one dword");
    asm volatile("global_load_dword %0, %1, off" : "=v"(dst) : "v"(src) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit count");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// (one statement per register or register group: a statement takes at most 30 operands, a column block has ten)
template <class V>
__device__ __forceinline__ void tie_loaded(V& v) {
    asm volatile("" : "+v"(v) : : "memory");
}
template <class V, int N>
__device__ __forceinline__ void tie_loaded(V (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) tie_loaded(v[i]);
}

}  // namespace vs
