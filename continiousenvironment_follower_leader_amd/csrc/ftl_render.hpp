// ftl_render.hpp -- ftl_render (include/ftl.h): batched top-down RGB frames of the reference's _show_tick (ENV:1229-1281).
// Included from ftl_abi.hip after the handle definition (same translation unit).
//
// Two launches on the caller's stream:
//   ftl_render_list_kernel -- one wavefront per requested env: the env's primitives in painter's order into its slice of the workspace.
//       Geometry is computed in float64 from the state and the scenario pool, then stored once as float32 output-pixel coordinates.
//   ftl_render_tile_kernel -- one workgroup of 256 lanes per 32 x 32 tile of one image, 4 consecutive pixels per lane.  The env's list is
//       culled by bounding box into LDS (order-preserving ballot / prefix compaction, in chunks of FTL_RENDER_CHUNK from the back), and
//       every lane walks the culled list back to front and stops at the first primitive that covers each of its pixels.  A lane's 4
//       pixels are one 12-byte store when the row pitch and the base allow it.
// Neither kernel writes anything but the workspace and the image.
#pragma once

#define FTL_RENDER_TILE 32
#define FTL_RENDER_THREADS 256
#define FTL_RENDER_CHUNK 512        // primitives staged in LDS at a time (16 KiB)

namespace ftlr {

enum { PRIM_DISC = 1, PRIM_SEG = 2, PRIM_RRECT = 3, PRIM_OUTLINE = 4 };

// 32 bytes.  g[] by type (output pixels):
//   DISC     cx, cy, r, r_in (< 0: filled disc; else a ring r_in < d <= r)
//   SEG      ax, ay, bx, by, half width
//   RRECT    cx, cy, ux, uy, hw, hh
//   OUTLINE  x0, y0, x1, y1 (the rect [x0, x1) x [y0, y1))
struct __align__(16) Prim { float g[7]; uint32_t meta; };   // meta = type << 24 | 0xRRGGBB

struct Args {
    int32_t width, height;
    float scale, ox, oy;
    uint32_t layers;
    int32_t k, cap;
    const int32_t* env_ids;
    const float* lasers;            // last ftl_outputs.lasers of the handle (may be NULL: no hit discs)
    Prim* prims;                    // [k][cap]
    int32_t* counts;                // [k]
    uint8_t* rgb;
    int32_t tiles_x, tiles_per_img;
    int32_t aligned;                // 12-byte groups may be stored as three dwords
};

// primitives per env the list kernel may write: route segments + 2 discs, green discs + ring, body + outline per object, per ray sensor a
// line per ray + a collide disc per ray and output row, tracker discs + 2 borders + 2 caps, target ring
inline int list_cap(const ftl_config& c, int R) {
    int rays = 0;
    for (int k = 0; k < c.n_lasers; k++) rays += c.lasers[k].count * (1 + c.lasers[k].history);
    return (c.route_cap + 2) + (c.traj_cap + 1) + 2 * (R + c.n_static) + rays + 3 * c.corr_cap + 2 + 1;
}

struct Geo {    // world -> output pixels (float64), stroke widths
    double ox, oy, inv;
    __device__ float X(double x) const { return (float)((x - ox) * inv); }
    __device__ float Y(double y) const { return (float)((y - oy) * inv); }
    __device__ float L(double r) const { return (float)(r * inv); }
    __device__ double W(double w) const { return fmax(w * inv, 1.0); }
};

__device__ __forceinline__ void put(Prim* p, int type, uint32_t rgb, float a, float b, float c, float d, float e = 0.f, float f = 0.f) {
    Prim q;
    q.g[0] = a; q.g[1] = b; q.g[2] = c; q.g[3] = d; q.g[4] = e; q.g[5] = f; q.g[6] = 0.f;
    q.meta = ((uint32_t)type << 24) | (rgb & 0xFFFFFFu);
    *p = q;
}
__device__ __forceinline__ void disc(Prim* p, const Geo& G, double x, double y, double r, uint32_t rgb) {
    put(p, PRIM_DISC, rgb, G.X(x), G.Y(y), G.L(r), -1.0f);
}
__device__ __forceinline__ void ring(Prim* p, const Geo& G, double x, double y, double r, double w, uint32_t rgb) {
    const double ro = r * G.inv, wo = G.W(w);
    put(p, PRIM_DISC, rgb, G.X(x), G.Y(y), (float)ro, (float)(ro - wo));
}
__device__ __forceinline__ void seg(Prim* p, const Geo& G, double ax, double ay, double bx, double by, double w, uint32_t rgb) {
    put(p, PRIM_SEG, rgb, G.X(ax), G.Y(ay), G.X(bx), G.Y(by), (float)(0.5 * G.W(w)));
}
__device__ __forceinline__ void robot(Prim* p, const Geo& G, double x, double y, double dir_deg, double w, double h, uint32_t rgb) {
    double s, c;
    ftl::sincos_bounded(dir_deg * ftl::kDeg2Rad, s, c);
    put(p, PRIM_RRECT, rgb, G.X(x), G.Y(y), (float)c, (float)s, G.L(0.5 * w), G.L(0.5 * h));
}
__device__ __forceinline__ void box(Prim* p, const Geo& G, const int32_t* r, uint32_t rgb) {      // filled axis-aligned int rect
    const double x = r[0], y = r[1], w = r[2], h = r[3];
    put(p, PRIM_RRECT, rgb, G.X(x + 0.5 * w), G.Y(y + 0.5 * h), 1.0f, 0.0f, G.L(0.5 * w), G.L(0.5 * h));
}
__device__ __forceinline__ void outline(Prim* p, const Geo& G, const int32_t* r) {
    const double x = r[0], y = r[1], w = r[2], h = r[3];
    put(p, PRIM_OUTLINE, FTL_RGB_RED, G.X(x), G.Y(y), G.X(x + w), G.Y(y + h));
}

__global__ void __launch_bounds__(FTL_WAVE) ftl_render_list_kernel(const FtlDevParams* __restrict__ dP, Args A) {
    const FtlDevParams& P = *dP;
    const ftl_config& c = P.cfg;
    const int j = blockIdx.x, lane = threadIdx.x;
    Prim* out = A.prims + (size_t)j * A.cap;
    const int e = A.env_ids[j];
    if (e < 0 || e >= P.n_envs) { if (lane == 0) A.counts[j] = 0; return; }
    const Geo G{(double)A.ox, (double)A.oy, 1.0 / (double)A.scale};
    const int32_t* ei = rec_field(P.env_int, P, e);
    const float* pos = rec_field(P.rb_pos, P, e);
    const double* rd = rec_field(P.rb_dbl, P, e);
    const int32_t* ri = rec_field(P.rb_int, P, e);
    const int R = P.R;
    const int s = ei[FTL_EI_SCEN];
    const bool have_s = s >= 0 && s < P.scen.n_scenarios;
    const int32_t* srect = have_s && c.n_static > 0 ? P.scen.static_rects + (size_t)s * c.n_static * 4 : nullptr;
    const double* route = have_s ? P.scen.route + (size_t)s * c.route_cap * 2 : nullptr;
    int rlen = have_s ? P.scen.route_len[s] : 0;
    rlen = rlen < 0 ? 0 : (rlen > c.route_cap ? c.route_cap : rlen);
    int n = 0;                                                             // wavefront-uniform write position
    const uint32_t L = A.layers;
    if (L & FTL_RENDER_PATH) {
        if (rlen > 2) {
            for (int i = lane; i < rlen - 1; i += FTL_WAVE)
                seg(out + n + i, G, route[2 * i], route[2 * i + 1], route[2 * i + 2], route[2 * i + 3], 1.0, FTL_RGB_RED);
            n += rlen - 1;
        }
        if (srect && c.n_static >= 2) {
            if (lane == 0) {
                const int32_t* a = srect; const int32_t* b = srect + 4;
                const double mx = ((a[0] + 0.5 * a[2]) + (b[0] + 0.5 * b[2])) * 0.5, my = ((a[1] + 0.5 * a[3]) + (b[1] + 0.5 * b[3])) * 0.5;
                disc(out + n, G, mx, my, 5.0, FTL_RGB_BLACK);
            }
            n += 1;
        }
        if (rlen >= 1) {
            if (lane == 0) disc(out + n, G, route[2 * (rlen - 1)], route[2 * (rlen - 1) + 1], 5.0, FTL_RGB_RED);
            n += 1;
        }
    }
    if (L & FTL_RENDER_BOX) {
        // the window _trajectory_in_box built (ENV:968-969, 1835-1841) over the trajectory as it was then: green_len points, the same
        // frame's append (ENV:1074-1075) came after it
        const int gl = ei[FTL_EI_GREEN_LEN], gc = ei[FTL_EI_GREEN_COUNT];
        if (gc > 5 && gl <= c.traj_cap && gl - 1 - gc >= 0) {
            const float* tr = P.traj + (size_t)e * c.traj_cap * 2;
            for (int i = lane; i < gc; i += FTL_WAVE) {                   // list order: green_len - 2 down to green_len - 1 - green_count
                const int q = gl - 2 - i;
                disc(out + n + i, G, (double)tr[2 * q], (double)tr[2 * q + 1], c.max_dev, FTL_RGB_GREEN);
            }
            n += gc;
        }
        if (lane == 0) ring(out + n, G, (double)pos[0], (double)pos[1], c.min_distance, ei[FTL_EI_TOO_CLOSE] ? 2.0 : 1.0, FTL_RGB_RED);
        n += 1;
    }
    if (L & FTL_RENDER_OBJECTS) {
        const bool rects = (L & FTL_RENDER_RECTS) != 0;
        const int per = rects ? 2 : 1;
        const int nobj = R + (srect ? c.n_static : 0);
        for (int o = lane; o < nobj; o += FTL_WAVE) {     // leader, follower, static rects, bears
            Prim* p = out + n + o * per;
            if (o < 2 || o >= 2 + (srect ? c.n_static : 0)) {
                const int r = o < 2 ? o : o - (srect ? c.n_static : 0);
                const ftl_robot_params& rp = r == 0 ? c.leader : (r == 1 ? c.follower : c.bear);
                robot(p, G, (double)pos[2 * r], (double)pos[2 * r + 1], rd[r * FTL_RD_COUNT + FTL_RD_DIRECTION], (double)rp.img_w, (double)rp.img_h,
                      r == 0 ? FTL_RGB_LEADER : (r == 1 ? FTL_RGB_FOLLOWER : FTL_RGB_BEAR));
                if (rects) outline(p + 1, G, ri + r * FTL_RI_COUNT);
            } else {
                const int32_t* sr = srect + (o - 2) * 4;
                box(p, G, sr, (o - 2) < 2 ? FTL_RGB_WALL : FTL_RGB_ROCK);
                if (rects) outline(p + 1, G, sr);
            }
        }
        n += nobj * per;
    }
    if (L & FTL_RENDER_SENSORS) {
        const double fx = pos[2], fy = pos[3], fdir = rd[FTL_RD_COUNT + FTL_RD_DIRECTION];
        for (int pass = 0; pass < 3; pass++) {
            if (pass == 1) {                                               // the v2 tracker
                if (c.has_tracker != 2) continue;
                const int lo = ei[FTL_EI_CORR_LO], hi = ei[FTL_EI_CORR_HI];
                int cnt = hi - lo;
                cnt = cnt < 0 ? 0 : (cnt > c.corr_cap ? c.corr_cap : cnt);
                const int m = c.corr_cap - 1;
                const double* hs = P.hist + (size_t)e * c.corr_cap * 2;
                const double* cr = P.corr + (size_t)e * c.corr_cap * 4;
                for (int i = lane; i < cnt; i += FTL_WAVE) {
                    const int q = (lo + i) & m;
                    disc(out + n + i, G, hs[2 * q], hs[2 * q + 1], 3.0, FTL_RGB_TRACK_HIST);
                }
                n += cnt;
                if (cnt > 1) {
                    for (int i = lane; i < 2 * (cnt - 1); i += FTL_WAVE) {  // right border, then left border
                        const int side = i >= cnt - 1 ? 1 : 0, t = i - side * (cnt - 1);
                        const int q0 = (lo + t) & m, q1 = (lo + t + 1) & m;
                        seg(out + n + i, G, cr[4 * q0 + 2 * side], cr[4 * q0 + 2 * side + 1], cr[4 * q1 + 2 * side], cr[4 * q1 + 2 * side + 1], 3.0, FTL_RGB_CORRIDOR);
                    }
                    n += 2 * (cnt - 1);
                    if (lane < 2) {
                        const int q = (lane == 0 ? lo : lo + cnt - 1) & m;
                        seg(out + n + lane, G, cr[4 * q], cr[4 * q + 1], cr[4 * q + 2], cr[4 * q + 3], 3.0, FTL_RGB_CORRIDOR);
                    }
                    n += 2;
                }
                continue;
            }
            for (int k = 0; k < c.n_lasers; k++) {
                const ftl_laser_cfg& l = c.lasers[k];
                if ((l.after_tracker != 0) != (pass == 2)) continue;
                const int N = l.count, H = l.history, Wd = N * (l.compas ? 5 : (l.pad_sectors ? 4 : 1));
                const double period = 360.0 / (double)N;
                // show() of LeaderCorridor_lasers / _v2 (SEN:728-733): lines and an r-5 disc at the current collide point of every ray;
                // of LeaderCorridor_Prev_lasers_v2 (SEN:970-985): lines, then per history row (oldest first) a disc at every ray's collide
                // point -- r 3 in the older rows, r 5 in the newest.  A collide point is the hit or, without one, the end point: the follower
                // plus the row's reading along the ray (the rows are scanned from the current position against older snapshots)
                const bool v1 = l.lenient || l.explicit_angles;
                const uint32_t line_rgb = v1 ? FTL_RGB_RAY_V2 : FTL_RGB_RAY;
                const int rows = (l.compas || A.lasers == nullptr) ? 0 : (v1 ? 1 : H);
                const float* blk = rows > 0 ? A.lasers + (size_t)e * P.lasers_len + l.out_offset : nullptr;
                for (int i = lane; i < N; i += FTL_WAVE) {
                    const double th = (l.explicit_angles ? (fdir + l.ray_angles[i & 7]) : ((fdir + l.angle_offset) + i * period)) * ftl::kDeg2Rad;
                    double sn, cs;
                    ftl::sincos_bounded(th, sn, cs);
                    seg(out + n + i, G, fx, fy, fx + cs * l.length, fy + sn * l.length, 1.0, line_rgb);
                }
                n += N;
                for (int m = lane; m < rows * N; m += FTL_WAVE) {
                    const int r = m / N, i = m - r * N, row = H - rows + r;
                    const double th = (l.explicit_angles ? (fdir + l.ray_angles[i & 7]) : ((fdir + l.angle_offset) + i * period)) * ftl::kDeg2Rad;
                    double sn, cs;
                    ftl::sincos_bounded(th, sn, cs);
                    int col = i;
                    if (l.pad_sectors) {
                        const double lis = (double)N / 4;
                        col = (((double)i < lis) ? 0 : ((double)i < 2 * lis) ? 1 : ((double)i < 3 * lis) ? 2 : 3) * N + i;
                    }
                    const double v = (double)blk[(size_t)row * Wd + col];
                    const bool newest = row == H - 1;
                    disc(out + n + m, G, fx + cs * v, fy + sn * v, newest ? 5.0 : 3.0,
                         v1 ? FTL_RGB_RAY_V2 : (newest ? FTL_RGB_RAY_HIT : FTL_RGB_RAY_HIT_OLD));
                }
                n += rows * N;
            }
        }
    }
    if (L & FTL_RENDER_TARGET) {
        if (lane == 0) {
            double tx, ty;
            if (rlen == 0) {
                const float* sp = have_s ? P.scen.robot_pos + (size_t)s * R * 2 : pos;       // the leader's start position
                tx = sp[0]; ty = sp[1];
            } else {
                int t = ei[FTL_EI_TARGET_ID];
                t = t < 0 ? 0 : (t > rlen - 1 ? rlen - 1 : t);
                tx = route[2 * t]; ty = route[2 * t + 1];
            }
            ring(out + n, G, tx, ty, 10.0, 2.0, FTL_RGB_RED);
        }
        n += 1;
    }
    if (lane == 0) A.counts[j] = n;
}

// bounding box test against the pixel centres [x0, x1] x [y0, y1] of a tile (conservative by a small margin)
__device__ __forceinline__ bool overlaps(const Prim& p, float x0, float y0, float x1, float y1) {
    const int t = (int)(p.meta >> 24);
    float a0, b0, a1, b1;
    const float m = 0.01f;
    if (t == PRIM_DISC) { a0 = p.g[0] - p.g[2]; a1 = p.g[0] + p.g[2]; b0 = p.g[1] - p.g[2]; b1 = p.g[1] + p.g[2]; }
    else if (t == PRIM_SEG) { a0 = fminf(p.g[0], p.g[2]) - p.g[4]; a1 = fmaxf(p.g[0], p.g[2]) + p.g[4];
                              b0 = fminf(p.g[1], p.g[3]) - p.g[4]; b1 = fmaxf(p.g[1], p.g[3]) + p.g[4]; }
    else if (t == PRIM_RRECT) { const float ex = fabsf(p.g[2]) * p.g[4] + fabsf(p.g[3]) * p.g[5], ey = fabsf(p.g[3]) * p.g[4] + fabsf(p.g[2]) * p.g[5];
                                a0 = p.g[0] - ex; a1 = p.g[0] + ex; b0 = p.g[1] - ey; b1 = p.g[1] + ey; }
    else if (t == PRIM_OUTLINE) { a0 = p.g[0]; a1 = p.g[2]; b0 = p.g[1]; b1 = p.g[3]; }
    else return false;
    return a1 + m >= x0 && a0 - m <= x1 && b1 + m >= y0 && b0 - m <= y1;
}

__device__ __forceinline__ bool covers(const Prim& p, float px, float py) {
    const int t = (int)(p.meta >> 24);
    if (t == PRIM_DISC) {
        const float dx = px - p.g[0], dy = py - p.g[1], d2 = dx * dx + dy * dy;
        return d2 <= p.g[2] * p.g[2] && (p.g[3] < 0.0f || d2 > p.g[3] * p.g[3]);
    }
    if (t == PRIM_SEG) {
        const float ex = p.g[2] - p.g[0], ey = p.g[3] - p.g[1], l2 = ex * ex + ey * ey;
        float u = l2 > 0.0f ? ((px - p.g[0]) * ex + (py - p.g[1]) * ey) / l2 : 0.0f;
        u = fminf(fmaxf(u, 0.0f), 1.0f);
        const float qx = (p.g[0] + u * ex) - px, qy = (p.g[1] + u * ey) - py;
        return qx * qx + qy * qy <= p.g[4] * p.g[4];
    }
    if (t == PRIM_RRECT) {
        const float dx = px - p.g[0], dy = py - p.g[1];
        const float a = dx * p.g[2] + dy * p.g[3], b = dy * p.g[2] - dx * p.g[3];
        return fabsf(a) <= p.g[4] && fabsf(b) <= p.g[5];
    }
    if (t == PRIM_OUTLINE) {
        if (!(px >= p.g[0] && px < p.g[2] && py >= p.g[1] && py < p.g[3])) return false;
        return px < p.g[0] + 1.0f || px >= p.g[2] - 1.0f || py < p.g[1] + 1.0f || py >= p.g[3] - 1.0f;
    }
    return false;
}

__global__ void __launch_bounds__(FTL_RENDER_THREADS) ftl_render_tile_kernel(Args A) {
    __shared__ Prim sp[FTL_RENDER_CHUNK];
    __shared__ int wtot[FTL_RENDER_THREADS / FTL_WAVE];
    const int tid = threadIdx.x, lane = tid & (FTL_WAVE - 1), wid = tid / FTL_WAVE;
    const int img = blockIdx.x / A.tiles_per_img, t = blockIdx.x - img * A.tiles_per_img;
    const int ty = t / A.tiles_x, tx = t - ty * A.tiles_x;
    const int bx = tx * FTL_RENDER_TILE, by = ty * FTL_RENDER_TILE;
    const int x0 = bx + (tid & 7) * 4, y = by + (tid >> 3);
    const float fx0 = bx + 0.5f, fy0 = by + 0.5f;
    const float fx1 = (float)min(bx + FTL_RENDER_TILE, A.width) - 0.5f, fy1 = (float)min(by + FTL_RENDER_TILE, A.height) - 0.5f;
    const Prim* list = A.prims + (size_t)img * A.cap;
    const int n = A.counts[img];
    uint32_t col[4] = {FTL_RGB_WHITE, FTL_RGB_WHITE, FTL_RGB_WHITE, FTL_RGB_WHITE};
    unsigned done = 0;
    for (int i = 0; i < 4; i++) if (x0 + i >= A.width || y >= A.height) done |= 1u << i;
    const float py = (float)y + 0.5f;
    for (int end = n; end > 0; end -= FTL_RENDER_CHUNK) {
        const int begin = end > FTL_RENDER_CHUNK ? end - FTL_RENDER_CHUNK : 0;
        if (__syncthreads_count(done != 0xFu) == 0) break;               // every pixel of the tile is decided
        int cnt = 0;                                                       // (uniform) primitives staged so far
        for (int base = begin; base < end; base += FTL_RENDER_THREADS) {
            const int i = base + tid;
            Prim p;
            bool keep = false;
            if (i < end) { p = list[i]; keep = overlaps(p, fx0, fy0, fx1, fy1); }
            const unsigned long long bal = __ballot(keep);
            const int before = __popcll(bal & ((1ull << lane) - 1ull));
            if (lane == 0) wtot[wid] = __popcll(bal);
            __syncthreads();
            int off = cnt, tot = 0;
            for (int w = 0; w < FTL_RENDER_THREADS / FTL_WAVE; w++) { if (w < wid) off += wtot[w]; tot += wtot[w]; }
            if (keep) sp[off + before] = p;
            cnt += tot;
            __syncthreads();
        }
        if (done != 0xFu) {
            for (int m = cnt - 1; m >= 0; m--) {
                const Prim p = sp[m];
                for (int q = 0; q < 4; q++)
                    if (!(done & (1u << q)) && covers(p, (float)(x0 + q) + 0.5f, py)) { col[q] = p.meta & 0xFFFFFFu; done |= 1u << q; }
                if (done == 0xFu) break;
            }
        }
        __syncthreads();                                                   // sp is rewritten by the next chunk
    }
    if (y >= A.height) return;
    uint8_t* row = A.rgb + ((size_t)img * A.height + y) * (size_t)A.width * 3;
    if (A.aligned && x0 + 3 < A.width) {
        // 4 pixels r g b -> 12 bytes little-endian in three dwords
        const uint32_t r0 = col[0] >> 16, g0 = (col[0] >> 8) & 255u, b0 = col[0] & 255u;
        const uint32_t r1 = col[1] >> 16, g1 = (col[1] >> 8) & 255u, b1 = col[1] & 255u;
        const uint32_t r2 = col[2] >> 16, g2 = (col[2] >> 8) & 255u, b2 = col[2] & 255u;
        const uint32_t r3 = col[3] >> 16, g3 = (col[3] >> 8) & 255u, b3 = col[3] & 255u;
        uint32_t* d = reinterpret_cast<uint32_t*>(row + (size_t)x0 * 3);
        d[0] = r0 | (g0 << 8) | (b0 << 16) | (r1 << 24);
        d[1] = g1 | (b1 << 8) | (r2 << 16) | (g2 << 24);
        d[2] = b2 | (r3 << 8) | (g3 << 16) | (b3 << 24);
    } else {
        for (int q = 0; q < 4; q++) {
            if (x0 + q >= A.width) break;
            uint8_t* d = row + (size_t)(x0 + q) * 3;
            d[0] = (uint8_t)(col[q] >> 16); d[1] = (uint8_t)(col[q] >> 8); d[2] = (uint8_t)col[q];
        }
    }
}

}  // namespace ftlr

extern "C" {

size_t ftl_sizeof_render_params(void) { return sizeof(ftl_render_params); }

static size_t render_ws_bytes(const ftl_handle* h, int32_t k, int* cap_out) {
    const int cap = ftlr::list_cap(h->P.cfg, h->P.R);
    if (cap_out) *cap_out = cap;
    return align_up((size_t)k * sizeof(int32_t), 256) + (size_t)k * (size_t)cap * sizeof(ftlr::Prim);
}

int ftl_render_workspace(const ftl_handle* h, int32_t k, size_t* bytes) {
    if (!h || !bytes) return fail(FTL_E_INVALID, "null argument");
    if (k <= 0) return fail(FTL_E_INVALID, "k must be positive");
    *bytes = render_ws_bytes(h, k, nullptr);
    return FTL_OK;
}

int ftl_render(ftl_handle* h, const int32_t* env_ids, int32_t k, const ftl_render_params* rp, void* workspace, size_t workspace_bytes,
               uint8_t* rgb, void* stream) {
    if (!h || !env_ids || !rp || !workspace || !rgb) return fail(FTL_E_INVALID, "null argument");
    if (k <= 0) return fail(FTL_E_INVALID, "k must be positive");
    if (rp->width <= 0 || rp->height <= 0) return fail(FTL_E_INVALID, "image size must be positive");
    if (!(rp->scale > 0.0f) || !std::isfinite(rp->scale) || !std::isfinite(rp->origin_x) || !std::isfinite(rp->origin_y))
        return fail(FTL_E_INVALID, "scale must be positive and finite, origin finite");
    if (rp->layers & ~FTL_RENDER_ALL) return fail(FTL_E_INVALID, "unknown layer bits");
    int cap = 0;
    if (workspace_bytes < render_ws_bytes(h, k, &cap)) return fail(FTL_E_INVALID, "render workspace too small (ftl_render_workspace)");
    const int tiles_x = (rp->width + FTL_RENDER_TILE - 1) / FTL_RENDER_TILE, tiles_y = (rp->height + FTL_RENDER_TILE - 1) / FTL_RENDER_TILE;
    const unsigned long long blocks = (unsigned long long)tiles_x * tiles_y * (unsigned long long)k;
    if (blocks * FTL_RENDER_THREADS > 0xFFFFFFFFull) return fail(FTL_E_INVALID, "k x image size too large for one launch");
    if (!h->bound) return fail(FTL_E_STATE, "ftl_bind_state has not been called");
    if (!h->have_scen) return fail(FTL_E_STATE, "ftl_load_scenarios has not been called");
    if (int rc = set_device(h)) return rc;
    { int rc = sync_params(h); if (rc) return rc; }
    ftlr::Args A;
    A.width = rp->width; A.height = rp->height; A.scale = rp->scale; A.ox = rp->origin_x; A.oy = rp->origin_y; A.layers = rp->layers;
    A.k = k; A.cap = cap; A.env_ids = env_ids; A.lasers = h->last_lasers;
    A.counts = (int32_t*)workspace;
    A.prims = (ftlr::Prim*)((char*)workspace + align_up((size_t)k * sizeof(int32_t), 256));
    A.rgb = rgb; A.tiles_x = tiles_x; A.tiles_per_img = tiles_x * tiles_y;
    A.aligned = (rp->width % 4 == 0 && ((uintptr_t)rgb & 3) == 0) ? 1 : 0;
    hipLaunchKernelGGL(ftlr::ftl_render_list_kernel, dim3((unsigned)k), dim3(FTL_WAVE), 0, (hipStream_t)stream, h->dP, A);
    hipLaunchKernelGGL(ftlr::ftl_render_tile_kernel, dim3((unsigned)blocks), dim3(FTL_RENDER_THREADS), 0, (hipStream_t)stream, A);
    return launched();
}

}  // extern "C"
