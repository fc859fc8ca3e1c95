// ftl_snapshot.hpp -- snapshot / clone / restore of env states (include/ftl.h: ftl_env_bytes .. ftl_unpack_envs_from).  Included at the end of
// ftl_abi.hip (same translation unit: it reads the handle's field table).
//
// One kernel, templated on the direction, moves env rows between the state buffer and a dense [k][env_bytes] row buffer.  An env is a
// short list of contiguous segments -- the used part of its record, then one row of every dense field -- described by a table built on
// the host from the frozen layout and passed in the kernarg segment.  A workgroup of 256 lanes covers FTL_SNAP_UNROLL * 256 16-byte
// chunks of one row (grid.y workgroups per row); every lane issues all its loads before its first store.  The table is read with
// compile-time indices only (no dynamically indexed kernarg array: that would go through scratch).
#include <hip/hip_runtime.h>

#define FTL_SNAP_MAX_SEGS 8       // the record + 7 dense fields
#define FTL_SNAP_THREADS 256
#define FTL_SNAP_UNROLL 4         // 16-byte chunks in flight per lane
#define FTL_ENV_ROW_FORMAT 1      // version of the row format (part of ftl_env_layout_id)

namespace ftls {

struct Seg {
    unsigned long long src_off;     // byte offset of env 0's bytes in the state buffer
    unsigned long long src_stride;  // bytes from one env to the next
    uint32_t row16;                 // first 16-byte chunk of the segment in the row
    uint32_t len;                   // bytes of the segment (the chunks past it in the row are zero padding)
    uint32_t vec;                   // 1: src_off, src_stride and len are multiples of 16 (whole-chunk vector copies); 0: 4-byte words
    uint32_t _pad;
};

struct Args {
    unsigned char* blob;            // the bound state buffer
    unsigned char* rows;            // [k][row_bytes]
    const int32_t* ids;             // [k] env indices of the handle
    const int32_t* row_ids;         // unpack: [k] env ids[i] takes row row_ids[i] (ftl_unpack_envs_from), or null: row i
    unsigned long long row_bytes;
    int32_t k, nseg, row16, env_id_base;
    uint32_t flags;                 // FTL_ENV_* (unpack)
    int32_t w_episodes, w_sticky, w_stream;   // row word index (4-byte units) of the env_int words the flags are about
    int32_t skip_seg;               // unpack without FTL_ENV_SLOT_STATS: index of the "ep_stats" segment (left as the destination has it)
    int32_t _pad;
    Seg seg[FTL_SNAP_MAX_SEGS];
};

// The segment of chunk c (a lane-varying choice among kernarg values read with constant indices).
struct Where { unsigned long long off, stride; uint32_t b, len, vec; int s; };

__device__ __forceinline__ Where locate(const Args& a, uint32_t c) {
    Where w{a.seg[0].src_off, a.seg[0].src_stride, c * 16u, a.seg[0].len, a.seg[0].vec, 0};
#pragma unroll
    for (int t = 1; t < FTL_SNAP_MAX_SEGS; t++)
        if (t < a.nseg && c >= a.seg[t].row16) {
            w.off = a.seg[t].src_off; w.stride = a.seg[t].src_stride; w.b = (c - a.seg[t].row16) * 16u; w.len = a.seg[t].len;
            w.vec = a.seg[t].vec; w.s = t;
        }
    return w;
}

// unpack: the destination's own value of a word the flags keep
__device__ __forceinline__ uint32_t merge_word(const Args& a, int wi, uint32_t row_v, uint32_t old_v, int env) {
    if (wi == a.w_stream) return (a.flags & FTL_ENV_OWN_STREAM) ? old_v : (uint32_t)((int32_t)row_v - a.env_id_base - env);
    if (wi == a.w_episodes || wi == a.w_sticky) return (a.flags & FTL_ENV_SLOT_STATS) ? row_v : old_v;
    return row_v;
}

template <bool UNPACK>
__global__ __launch_bounds__(FTL_SNAP_THREADS) void ftl_snapshot_kernel(Args a) {
    const int i = blockIdx.x;                                  // row i of the buffer <-> env a.ids[i]
    const int env = a.ids[i];
    const int ri = (UNPACK && a.row_ids) ? a.row_ids[i] : i;
    unsigned char* row = a.rows + (size_t)ri * a.row_bytes;
    const uint32_t c0 = blockIdx.y * (FTL_SNAP_THREADS * FTL_SNAP_UNROLL) + threadIdx.x;
    uint4 v[FTL_SNAP_UNROLL];
#pragma unroll
    for (int u = 0; u < FTL_SNAP_UNROLL; u++) {                // loads
        const uint32_t c = c0 + u * FTL_SNAP_THREADS;
        v[u] = make_uint4(0u, 0u, 0u, 0u);
        if (c >= (uint32_t)a.row16) continue;
        if (UNPACK) { v[u] = *reinterpret_cast<const uint4*>(row + (size_t)c * 16); continue; }
        const Where w = locate(a, c);
        if (w.b >= w.len) continue;                            // the row's tail padding stays zero
        const unsigned char* src = a.blob + w.off + (size_t)env * w.stride + w.b;
        if (w.vec) v[u] = *reinterpret_cast<const uint4*>(src);
        else {
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
            if (w.b + 4 <= w.len) v[u].x = s4[0];
            if (w.b + 8 <= w.len) v[u].y = s4[1];
            if (w.b + 12 <= w.len) v[u].z = s4[2];
            if (w.b + 16 <= w.len) v[u].w = s4[3];
        }
    }
#pragma unroll
    for (int u = 0; u < FTL_SNAP_UNROLL; u++) {                // stores
        const uint32_t c = c0 + u * FTL_SNAP_THREADS;
        if (c >= (uint32_t)a.row16) continue;
        const int wi = (int)(c * 4u);                          // row word index of v[u].x (the record is the row's first segment)
        auto hit = [&](int w) { return (unsigned)(w - wi) < 4u; };
        const bool special = hit(a.w_stream) || hit(a.w_episodes) || hit(a.w_sticky);
        if (!UNPACK) {
            if (hit(a.w_stream)) {                             // the row carries the absolute stream id
                const int j = a.w_stream - wi, add = a.env_id_base + env;
                v[u].x += j == 0 ? add : 0; v[u].y += j == 1 ? add : 0; v[u].z += j == 2 ? add : 0; v[u].w += j == 3 ? add : 0;
            }
            *reinterpret_cast<uint4*>(row + (size_t)c * 16) = v[u];
            continue;
        }
        const Where w = locate(a, c);
        if (w.s == a.skip_seg || w.b >= w.len) continue;
        unsigned char* dst = a.blob + w.off + (size_t)env * w.stride + w.b;
        if (w.s == 0 && special) {                             // chunk of the record with a word the flags are about: merge with the old one
            const uint4 o = *reinterpret_cast<const uint4*>(dst);
            v[u].x = merge_word(a, wi, v[u].x, o.x, env); v[u].y = merge_word(a, wi + 1, v[u].y, o.y, env);
            v[u].z = merge_word(a, wi + 2, v[u].z, o.z, env); v[u].w = merge_word(a, wi + 3, v[u].w, o.w, env);
        }
        if (w.vec) *reinterpret_cast<uint4*>(dst) = v[u];
        else {
            uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
            if (w.b + 4 <= w.len) d4[0] = v[u].x;
            if (w.b + 8 <= w.len) d4[1] = v[u].y;
            if (w.b + 12 <= w.len) d4[2] = v[u].z;
            if (w.b + 16 <= w.len) d4[3] = v[u].w;
        }
    }
}

// the segment table of a handle (host): record first, then the dense fields in ftl_state_field order
static Args make_args(const ftl_handle* h) {
    Args a;
    memset(&a, 0, sizeof a);
    size_t rec_used = 0;
    for (int i = 0; i < FTL_N_FIELDS; i++) {
        const Field& f = h->fields[i];
        const size_t esz = f.dtype == 2 ? 8 : 4;
        if (f.offset < (size_t)h->P.rec_stride) {                                     // a record field (record 0 starts the buffer)
            const size_t end = align_up(f.offset + f.per_env * esz, 16);
            rec_used = end > rec_used ? end : rec_used;
        }
    }
    a.seg[0] = Seg{0ull, (unsigned long long)h->P.rec_stride, 0u, (uint32_t)rec_used, 1u, 0u};
    int ns = 1;
    size_t row = rec_used;
    a.skip_seg = -1;
    for (int i = 0; i < FTL_N_FIELDS; i++) {
        const Field& f = h->fields[i];
        const size_t esz = f.dtype == 2 ? 8 : 4;
        if (f.offset < (size_t)h->P.rec_stride || f.per_env == 0) continue;       // record fields (above) and empty fields
        const size_t len = f.per_env * esz;
        if (!strcmp(f.name, "ep_stats")) a.skip_seg = ns;
        const bool vec = f.offset % 16 == 0 && f.stride % 16 == 0 && len % 16 == 0;
        a.seg[ns++] = Seg{(unsigned long long)f.offset, (unsigned long long)f.stride, (uint32_t)(row / 16), (uint32_t)len, vec ? 1u : 0u, 0u};
        row = align_up(row + len, 16);
    }
    a.nseg = ns;
    a.row_bytes = align_up(row, 256);
    a.row16 = (int32_t)(a.row_bytes / 16);
    a.env_id_base = h->P.cfg.env_id_base;
    const size_t w0 = h->fields[F_env_int].offset / 4;                 // env_int (record-relative: record 0 sits at offset 0)
    a.w_episodes = (int32_t)(w0 + FTL_EI_EPISODES); a.w_sticky = (int32_t)(w0 + FTL_EI_ERROR_STICKY); a.w_stream = (int32_t)(w0 + FTL_EI_STREAM);
    return a;
}

static int snap_launch(const ftl_handle* h, Args& a, bool unpack, void* stream) {
    if (int rc = set_device(h)) return rc;
    const unsigned per_wg = FTL_SNAP_THREADS * FTL_SNAP_UNROLL;
    const dim3 grid((unsigned)a.k, (unsigned)((a.row16 + per_wg - 1) / per_wg)), block(FTL_SNAP_THREADS);
    if (unpack) hipLaunchKernelGGL(ftl_snapshot_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(ftl_snapshot_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
    return launched();
}

static int snap_check(const ftl_handle* h, const int32_t* env_ids, int32_t k, const void* rows, uint32_t flags) {
    if (!h) return fail(FTL_E_INVALID, "null argument");
    if (flags & ~(FTL_ENV_SLOT_STATS | FTL_ENV_OWN_STREAM)) return fail(FTL_E_INVALID, "unknown ftl_unpack_envs flag bits");
    if (k < 0) return fail(FTL_E_INVALID, "k < 0");
    if (k > 0 && (!env_ids || !rows)) return fail(FTL_E_INVALID, "null env_ids / rows");
    if (((uintptr_t)rows) & 15) return fail(FTL_E_INVALID, "rows must be 16-byte aligned");
    if (!h->bound) return fail(FTL_E_STATE, "ftl_bind_state has not been called");
    return FTL_OK;
}

}  // namespace ftls

extern "C" {

size_t ftl_env_bytes(const ftl_handle* h) { return h ? (size_t)ftls::make_args(h).row_bytes : 0; }

uint64_t ftl_env_layout_id(const ftl_handle* h) {
    if (!h) return 0;
    ftl_config c = h->P.cfg;                                   // the frozen config (out_offset filled in) without the shard's position
    c.env_id_base = 0;
    uint64_t x = 0xcbf29ce484222325ULL;                        // FNV-1a 64
    auto mix = [&](const void* p, size_t n) { for (size_t i = 0; i < n; i++) { x ^= ((const unsigned char*)p)[i]; x *= 0x100000001b3ULL; } };
    const int32_t ver[2] = {FTL_ABI_VERSION, FTL_ENV_ROW_FORMAT};
    const uint64_t eb = (uint64_t)ftl_env_bytes(h);
    mix(ver, sizeof ver); mix(&eb, sizeof eb); mix(&c, sizeof c);
    return x;
}

int ftl_pack_envs(const ftl_handle* h, const int32_t* env_ids, int32_t k, void* rows, void* stream) {
    int rc = ftls::snap_check(h, env_ids, k, rows, 0u);
    if (rc || k == 0) return rc;
    ftls::Args a = ftls::make_args(h);
    a.blob = (unsigned char*)h->P.env_int - h->fields[F_env_int].offset; a.rows = (unsigned char*)rows; a.ids = env_ids; a.k = k;
    return ftls::snap_launch(h, a, false, stream);
}

int ftl_unpack_envs_from(ftl_handle* h, const void* rows, const int32_t* row_ids, const int32_t* env_ids, int32_t k, uint32_t flags, void* stream) {
    int rc = ftls::snap_check(h, env_ids, k, rows, flags);
    if (rc || k == 0) return rc;
    ftls::Args a = ftls::make_args(h);
    a.blob = (unsigned char*)h->P.env_int - h->fields[F_env_int].offset; a.rows = (unsigned char*)rows; a.ids = env_ids; a.row_ids = row_ids; a.k = k;
    a.flags = flags;
    if (flags & FTL_ENV_SLOT_STATS) a.skip_seg = -1;
    return ftls::snap_launch(h, a, true, stream);
}

int ftl_unpack_envs(ftl_handle* h, const void* rows, const int32_t* env_ids, int32_t k, uint32_t flags, void* stream) {
    return ftl_unpack_envs_from(h, rows, nullptr, env_ids, k, flags, stream);
}

}  // extern "C"
