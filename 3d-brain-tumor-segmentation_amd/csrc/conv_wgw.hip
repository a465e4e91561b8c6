// Weight gradient of the 3x3x3 stride-1 convolution in Winograd form with all three axes transformed, F(2x2x2, 3x3x3) -- the
// counterpart of conv_wino3.hip for  dW[kz,ky,kx,c,k] = sum_v P[v + (kz-1,ky-1,kx-1)][c] * Q[v][k]:
//   dW = (G^T x G^T x G^T) sum over 2x2x2 patches of  [ (B^T x B^T x B^T) P_4x4x4 ] o [ (A x A x A) Q_2x2x2 ]
// (B^T, G, A^T as in conv_wino3.hip's header; P = x with a one-voxel halo, Q = dy).  64 accumulator tiles, each fed one
// patch = 8 voxels at a time: 8/27 of the direct form's matrix instructions.  The contraction runs over patches, so channels
// sit on the lanes.  4 waves = the 4 xi_z, each 16 accumulators (xi_y, xi_x) = 256 registers, one wave per SIMD.
// Lane = (channel, patch parity): the K = 2 of an instruction is two x-neighbouring patches, so the sub-tile 16 x 4 x 2 = 16
// patches (the direct kernel's: plan, partial layout [27 taps][32][32] per workgroup and finalize kernels are shared) is 8 steps
// of 16 matrix instructions.  LDS tiles are x-fastest, [row][channel][18], transposed while staging: P rows hold x = -1..16, Q
// rows x = 0..15 (+2 unused).  A lane's four x inputs of a patch are two 8-byte reads at an 8-byte-aligned offset; the row
// stride of 18 floats sends the 32 channels of a half wave to 32 distinct bank pairs ((9 c) mod 32 is a permutation):
// conflict-free.  Staging slots run channel quad fastest, then x: a wave's 16-byte loads are contiguous in memory and its
// transposing 4-byte LDS writes hit banks 8 cq + x (8 x 8 distinct).  The z combination of P is taken on the way into LDS, as
// w3_kernel's commit() does: a thread stages the four z rows of one column and writes the planes d0 - d2 | d1 + d2 | d2 - d1 |
// d1 - d3 into the rows of the four z rows, a wave reads the plane of its own xi_z and transforms y and x.  Q stays raw (its
// planes would not fit); xi = 3 of Q carries +q1 for the true -q1 on every axis, undone where G^T is applied (in the wave for y
// and x, across the waves through LDS for z).  Every step is branch-free: the next sub-tile's loads go through descriptors that
// are empty behind the workgroup's last sub-tile, and everything a step consumes was asked for two steps earlier (global loads
// before their LDS writes, LDS reads before their matrix instructions).  Bias partials: the all-sum point of Q (xi = 1 on every
// axis, wave 1).
#include "wgrad_plan.h"

typedef float wg_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ wg_f32x2 wgw_pk_add(wg_f32x2 a, wg_f32x2 b) { wg_f32x2 d; asm("v_pk_add_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ wg_f32x2 wgw_pk_sub(wg_f32x2 a, wg_f32x2 b) { wg_f32x2 d; asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ wg_f32x2 wgw_pk_fma(wg_f32x2 a, wg_f32x2 b, wg_f32x2 c) { wg_f32x2 d; asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c)); return d; }
// (a.x + b.y, a.x - b.y)
__device__ __forceinline__ wg_f32x2 wgw_pk_addsub(wg_f32x2 a, wg_f32x2 b) { wg_f32x2 d; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ float wgw_acc_rd(float a) { float v; asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a)); return v; }

#define WGW_THREADS 256
#define WGW_RS 18
#define WGW_PTILE (24 * 32 * WGW_RS)         /* 4 z-rows x 6 y-rows */
#define WGW_QTILE (8 * 32 * WGW_RS)          /* 2 z-rows x 4 y-rows */
#define WGW_BUF (WGW_PTILE + WGW_QTILE)      /* 18432 floats = 72 KB, double buffered; the two = the 4 x 9 tiles of the combine */
#define WGW_PLANE (6 * 32 * WGW_RS)          /* one xi_z plane of the P tile: 6 y-rows */
#define WGW_NPC 4                            /* P column slots per thread: 6 y-rows x 18 x x 8 channel quads = 864 = 3.375 x 256 */
#define WGW_NQS 4                            /* Q slots per thread: 8 rows x 16 x x 8 channel quads = 1024 */

__global__ __launch_bounds__(WGW_THREADS, 1) void wgw_kernel(const WgradParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // = xi_z
  const int ch = lane & 31, hh = lane >> 5;
  const int pct = blockIdx.y, qct = blockIdx.z;
  const float* pP = p.p + pct * 32;
  const float* pQ = p.q + qct * 32;

  // ---- staging maps.  P: column id = tid + 256*i = ((y row * 18) + x) * 8 + channel quad; a thread loads the four z rows of its
  //      column, each through the descriptor of that z row, and writes the four xi_z planes.  Byte offsets relative to the z row's
  //      origin are computed once; a column on a y or x face of the image gets a 2 GB offset = outside the descriptor, the load
  //      returns zeros (4 face bits per column against 4 per tile); a z row outside the image has an empty descriptor.
  //      Q: slot id = tid + 256*i = ((row * 16) + x) * 8 + channel quad, raw. ----
  int c_lds[WGW_NPC - 1], c3_lds[4];
  unsigned coff[WGW_NPC], cfl = 0u;
#pragma unroll
  for (int i = 0; i < WGW_NPC; ++i) {
    const int id = tid + WGW_THREADS * i;
    int l = 0;
    coff[i] = 0x80000000u;
    if (id < 6 * 18 * 8) {
      const int cq = id & 7, vox = id >> 3;
      const int yr = vox / 18, xx = vox - yr * 18;
      l = (yr * 32 + cq * 4) * WGW_RS + xx;
      coff[i] = (unsigned)((yr * p.Wp + xx) * p.ldp + cq * 4) * 4u;
      const unsigned fl = (yr == 0 ? 1u : 0u) | (yr == 5 ? 2u : 0u) | (xx == 0 ? 4u : 0u) | (xx == 17 ? 8u : 0u);
      cfl |= fl << (4 * i);
    }
    if (i < WGW_NPC - 1) {
      c_lds[i < WGW_NPC - 1 ? i : 0] = l;
    } else {
      // (the partly filled last slot: its idle threads load nothing and write their zeros to the unused x = 16, 17 of the Q rows,
      // four channels of one row per plane)
      const int idle = id - 6 * 18 * 8;
#pragma unroll
      for (int pl = 0; pl < 4; ++pl)
        c3_lds[pl] = idle < 0 ? l + pl * WGW_PLANE : WGW_PTILE + 4 * (((idle >> 1) + 16 * pl) & 63) * WGW_RS + 16 + (idle & 1);
    }
  }
  int q_lds[WGW_NQS];
  unsigned qoff[WGW_NQS];
#pragma unroll
  for (int i = 0; i < WGW_NQS; ++i) {
    const int id = tid + WGW_THREADS * i;
    const int cq = id & 7, xx = (id >> 3) & 15, row = id >> 7;   // row = oz*4 + oy
    q_lds[i] = WGW_PTILE + (row * 32 + cq * 4) * WGW_RS + xx;
    qoff[i] = (unsigned)((((row >> 2) * p.Hq + (row & 3)) * p.Wq + xx) * p.ldq + cq * 4) * 4u;
  }
  const int t0 = blockIdx.x * p.sub_per_wg;
  int t1 = t0 + p.sub_per_wg;
  if (t1 > p.nsub) t1 = p.nsub;
  // coordinates and origins (P: the halo corner) of the NEXT sub-tile to fetch.  Sub-tiles of a workgroup are consecutive: the
  // coordinates advance by carries and the origins by 32-bit byte strides, no division or 64-bit product in the loop
  int ftx, fty, ftz, fn;
  {
    int t = t0;
    ftx = t % p.ntx; t /= p.ntx;
    fty = t % p.nty; t /= p.nty;
    ftz = t % p.ntz;
    fn = t / p.ntz;
  }
  const char* f_pb = reinterpret_cast<const char*>(pP + ((((long)fn * p.Dp + 2 * ftz - 1) * p.Hp + 4 * fty - 1) * p.Wp + 16 * ftx - 1) * p.ldp);
  const char* f_qb = reinterpret_cast<const char*>(pQ + ((((long)fn * p.Dq + 2 * ftz) * p.Hq + 4 * fty) * p.Wq + 16 * ftx) * p.ldq);
  const long zrow = (long)p.Hp * p.Wp * p.ldp;
  // bytes to the next sub-tile along x; more to the first of the next y row; more to the first of the next z row (tiles are whole
  // and samples contiguous: the next sample's first is one more z row on).  The launcher keeps five z rows of P and three of Q
  // below 2 GB.
  const unsigned pdx = 64u * p.ldp, pdy = 12u * p.Wp * p.ldp, pdz = (unsigned)zrow * 4u;
  const unsigned qdx = 64u * p.ldq, qdy = 12u * p.Wq * p.ldq, qdz = (unsigned)p.Hq * p.Wq * p.ldq * 4u;
  // The 20 requests of the next sub-tile go out in six groups (P column 0 | 1 | 2 | 3, four z rows each | Q 0-1 | Q 2-3).  Group k is
  // written to the OTHER LDS buffer at step k and requested two steps before that -- groups 0 and 1 in the last two steps of the
  // sub-tile before, where fetch_begin has just made its descriptors: a request has two steps to come back before the in-order
  // wait of its write.
  f32x4 pre[4 * WGW_NPC + WGW_NQS];
  __amdgpu_buffer_rsrc_t f_pr[4], f_qr;
  unsigned f_cm[WGW_NPC] = {0u, 0u, 0u, 0u};   // the tile's y / x face bits at the place of each column's
  auto fetch_begin = [&](bool live) {   // live = false: empty descriptors, every load returns zeros without traffic
    const float* pb = reinterpret_cast<const float*>(f_pb);
    const float* qb = reinterpret_cast<const float*>(f_qb);
    f_pr[0] = __builtin_amdgcn_make_buffer_rsrc((void*)pb, 0, (live && ftz != 0) ? 0x7fffffff : 0, 0x00020000);
    f_pr[1] = __builtin_amdgcn_make_buffer_rsrc((void*)(pb + zrow), 0, live ? 0x7fffffff : 0, 0x00020000);
    f_pr[2] = __builtin_amdgcn_make_buffer_rsrc((void*)(pb + 2 * zrow), 0, live ? 0x7fffffff : 0, 0x00020000);
    f_pr[3] = __builtin_amdgcn_make_buffer_rsrc((void*)(pb + 3 * zrow), 0, (live && ftz != p.ntz - 1) ? 0x7fffffff : 0, 0x00020000);
    f_qr = __builtin_amdgcn_make_buffer_rsrc((void*)qb, 0, live ? 0x7fffffff : 0, 0x00020000);
    const unsigned tm = (fty == 0 ? 1u : 0u) | (fty == p.nty - 1 ? 2u : 0u) | (ftx == 0 ? 4u : 0u) | (ftx == p.ntx - 1 ? 8u : 0u);
#pragma unroll
    for (int i = 0; i < WGW_NPC; ++i) f_cm[i] = tm << (4 * i);
    const int cx = (ftx + 1 == p.ntx) ? 1 : 0;   // (selects, no branches: the call sits inside a scheduled step)
    ftx = cx ? 0 : ftx + 1;
    const int cy = (fty + cx == p.nty) ? 1 : 0;
    fty = cy ? 0 : fty + cx;
    const int cz = (ftz + cy == p.ntz) ? 1 : 0;
    ftz = cz ? 0 : ftz + cy;
    f_pb += pdx + cx * pdy + cy * pdz;   // (cy implies cx)
    f_qb += qdx + cx * qdy + cy * qdz;
  };
  auto load4 = [](__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
  };
  auto sub4 = [](f32x4 a, f32x4 b) {
    const wg_f32x2 lo = wgw_pk_sub(a.xy, b.xy), hi = wgw_pk_sub(a.zw, b.zw);
    return f32x4{lo.x, lo.y, hi.x, hi.y};
  };
  auto add4 = [](f32x4 a, f32x4 b) {
    const wg_f32x2 lo = wgw_pk_add(a.xy, b.xy), hi = wgw_pk_add(a.zw, b.zw);
    return f32x4{lo.x, lo.y, hi.x, hi.y};
  };
  auto fetch_group = [&](auto kc) {
    constexpr int k = decltype(kc)::value;
    if constexpr (k < WGW_NPC) {
      const unsigned off = (cfl & f_cm[k]) ? 0x80000000u : coff[k];
#pragma unroll
      for (int zr = 0; zr < 4; ++zr) pre[4 * k + zr] = load4(f_pr[zr], off);
    } else {
      constexpr int i = 2 * (k - WGW_NPC);
      pre[4 * WGW_NPC + i] = load4(f_qr, qoff[i]);
      pre[4 * WGW_NPC + i + 1] = load4(f_qr, qoff[i + 1]);
    }
  };
  auto commit_group = [&](float* buf, auto kc) {
    constexpr int k = decltype(kc)::value;
    if constexpr (k < WGW_NPC) {   // xi_z planes d0 - d2 | d1 + d2 | d2 - d1 | d1 - d3 of the column, into the rows of the four z rows
      const f32x4 d0 = pre[4 * k], d1 = pre[4 * k + 1], d2 = pre[4 * k + 2], d3 = pre[4 * k + 3];
      const f32x4 pl[4] = {sub4(d0, d2), add4(d1, d2), sub4(d2, d1), sub4(d1, d3)};
#pragma unroll
      for (int z = 0; z < 4; ++z) {
        float* o;
        if constexpr (k < WGW_NPC - 1) o = buf + c_lds[k] + z * WGW_PLANE;
        else o = buf + c3_lds[z];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e * WGW_RS] = pl[z][e];
      }
    } else {
      constexpr int i0 = 2 * (k - WGW_NPC);
#pragma unroll
      for (int i = i0; i < i0 + 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) buf[q_lds[i] + e * WGW_RS] = pre[4 * WGW_NPC + i][e];
    }
  };
  // the staging share of step s: write group s (steps 0-5: the barrier sits before step 6), request the group that is written two
  // steps on.  The descriptors of the sub-tile after the next (live2: it exists) are made in step 6, which requests its group 0,
  // behind the last request of the next (group 5, step 3)
  auto stage = [&](float* buf, auto sc, bool live2) {
    constexpr int s = decltype(sc)::value;
    if constexpr (s <= 5) commit_group(buf, IC<s>{});
    if constexpr (s == 6) fetch_begin(live2);
    if constexpr (s + 2 <= 5) fetch_group(IC<s + 2>{});
    else if constexpr (s >= 6) fetch_group(IC<s - 6>{});
  };

  // ---- wave roles: xi_z of P: the wave's own plane; of Q: a = X + sq * Y (xi_z = 3: +q1) ----
  const float sq = (wave == 1) ? 1.f : (wave == 2) ? -1.f : 0.f;
  const wg_f32x2 sq2 = {sq, sq};
  const int pA = wave * WGW_PLANE + ch * WGW_RS + 2 * hh;
  const int qXa = WGW_PTILE + ((wave == 3 ? 4 : 0) * 32 + ch) * WGW_RS + 2 * hh;
  const int qYa = WGW_PTILE + (4 * 32 + ch) * WGW_RS + 2 * hh;
  const bool bias = p.want_bias && pct == 0 && wave == 1;
  double bsum = 0.0;
  float bs = 0.f;   // the all-sum point of Q (xi = 1 on every axis; wave 1) over one sub-tile

  f32x16 acc[4][4];   // [xi_y][xi_x]
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;

  struct WgwOps { float v[4][4], t[4][4]; };
  struct WgwRaw { wg_f32x2 pl[4], px[4], qx[2], qy[2]; };
  // LDS reads of step st = (patch row py, x patch pair sx): this lane's patch is px = 2 sx + hh.  They are issued two steps before
  // the matrix instructions that use them and transformed one step before: a read has a whole step to come back
  auto rd = [&](const float* cur, auto stc, WgwRaw& r) {
    constexpr int st = decltype(stc)::value;
    constexpr int py = st >> 2, sx = st & 3;
#pragma unroll
    for (int yr = 0; yr < 4; ++yr) {   // rows of the wave's xi_z plane: x inputs 0,1 | 2,3
      const float* a = cur + pA + (2 * py + yr) * 32 * WGW_RS + 4 * sx;
      r.pl[yr] = *reinterpret_cast<const wg_f32x2*>(a);
      r.px[yr] = *reinterpret_cast<const wg_f32x2*>(a + 2);
    }
#pragma unroll
    for (int yr = 0; yr < 2; ++yr) {
      r.qx[yr] = *reinterpret_cast<const wg_f32x2*>(cur + qXa + (2 * py + yr) * 32 * WGW_RS + 4 * sx);
      r.qy[yr] = *reinterpret_cast<const wg_f32x2*>(cur + qYa + (2 * py + yr) * 32 * WGW_RS + 4 * sx);
    }
  };
  auto xf = [&](const WgwRaw& r, WgwOps& o) {
    wg_f32x2 vl[4], vx[4];
    vl[0] = wgw_pk_sub(r.pl[0], r.pl[2]); vx[0] = wgw_pk_sub(r.px[0], r.px[2]);
    vl[1] = wgw_pk_add(r.pl[1], r.pl[2]); vx[1] = wgw_pk_add(r.px[1], r.px[2]);
    vl[2] = wgw_pk_sub(r.pl[2], r.pl[1]); vx[2] = wgw_pk_sub(r.px[2], r.px[1]);
    vl[3] = wgw_pk_sub(r.pl[1], r.pl[3]); vx[3] = wgw_pk_sub(r.px[1], r.px[3]);
#pragma unroll
    for (int a = 0; a < 4; ++a) {   // x: e0 - e2 | e1 + e2 | e2 - e1 | e1 - e3
      const wg_f32x2 d = wgw_pk_sub(vl[a], vx[a]), m = wgw_pk_addsub(vx[a], vl[a]);
      o.v[a][0] = d.x;
      o.v[a][1] = m.x;
      o.v[a][2] = m.y;
      o.v[a][3] = d.y;
    }
    const wg_f32x2 qa[2] = {wgw_pk_fma(r.qy[0], sq2, r.qx[0]), wgw_pk_fma(r.qy[1], sq2, r.qx[1])};
    const wg_f32x2 ty[4] = {qa[0], wgw_pk_add(qa[0], qa[1]), wgw_pk_sub(qa[0], qa[1]), qa[1]};
#pragma unroll
    for (int a = 0; a < 4; ++a) {   // x: e0 | e0 + e1 | e0 - e1 | + e1
      const wg_f32x2 m = wgw_pk_addsub(ty[a], ty[a]);
      o.t[a][0] = ty[a].x;
      o.t[a][1] = m.x;
      o.t[a][2] = m.y;
      o.t[a][3] = ty[a].y;
    }
    bs += o.t[1][1];
  };
  auto mfma16 = [&](const WgwOps& o) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.v[a][b], o.t[a][b], acc[a][b], 0, 0, 0);
  };
  // one slot of the schedule per matrix instruction: the MFMA, then up to four vector-ALU operations and three memory operations
  // of the work that shares the step (next step's operands, the staging group)
#define WGW_SCHED_STEP()                                   \
  _Pragma("unroll") for (int q_ = 0; q_ < 16; ++q_) {      \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     \
    __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);     \
    __builtin_amdgcn_sched_group_barrier(0x320, 3, 0);     \
  }
#define WGW_STEP_END()                       \
  WGW_SCHED_STEP();                          \
  __builtin_amdgcn_sched_barrier(0);         \
  asm volatile("s_nop 1" ::: "memory");   /* hand-written VALU -> MFMA operand: the compiler does not track that hazard */

  fetch_begin(t0 < t1);
  fetch_group(IC<0>{}); fetch_group(IC<1>{}); fetch_group(IC<2>{}); fetch_group(IC<3>{}); fetch_group(IC<4>{}); fetch_group(IC<5>{});
  commit_group(lds, IC<0>{}); commit_group(lds, IC<1>{}); commit_group(lds, IC<2>{}); commit_group(lds, IC<3>{});
  commit_group(lds, IC<4>{}); commit_group(lds, IC<5>{});
  __syncthreads();
  WgwOps opA, opB;
  WgwRaw rawA, rawB;
  // (in the order of the loop's last two steps, so that the waits counted behind the loop's head are the same on both ways in)
  rd(lds, IC<0>{}, rawA);
  __builtin_amdgcn_sched_barrier(0);
  fetch_begin((t0 + 1) < t1);
  fetch_group(IC<0>{});
  __builtin_amdgcn_sched_barrier(0);
  rd(lds, IC<1>{}, rawB);
  __builtin_amdgcn_sched_barrier(0);
  xf(rawA, opA);
  __builtin_amdgcn_sched_barrier(0);
  fetch_group(IC<1>{});
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 3" ::: "memory");
  // step s: the matrix instructions of step s, the transform of step s + 1, the LDS reads of step s + 2, the staging share
  for (int t = t0; t < t1; ++t) {
    const float* cur = lds + ((t - t0) & 1) * WGW_BUF;
    float* nxt = lds + ((t - t0 + 1) & 1) * WGW_BUF;
    const bool live2 = (t + 2) < t1;
    rd(cur, IC<2>{}, rawA); xf(rawB, opB); stage(nxt, IC<0>{}, live2);
    mfma16(opA);
    WGW_STEP_END();
    rd(cur, IC<3>{}, rawB); xf(rawA, opA); stage(nxt, IC<1>{}, live2);
    mfma16(opB);
    WGW_STEP_END();
    rd(cur, IC<4>{}, rawA); xf(rawB, opB); stage(nxt, IC<2>{}, live2);
    mfma16(opA);
    WGW_STEP_END();
    rd(cur, IC<5>{}, rawB); xf(rawA, opA); stage(nxt, IC<3>{}, live2);
    mfma16(opB);
    WGW_STEP_END();
    rd(cur, IC<6>{}, rawA); xf(rawB, opB); stage(nxt, IC<4>{}, live2);
    mfma16(opA);
    WGW_STEP_END();
    rd(cur, IC<7>{}, rawB); xf(rawA, opA); stage(nxt, IC<5>{}, live2);
    mfma16(opB);
    WGW_STEP_END();
    // the barrier sits before step 6: the reads of the next sub-tile's steps 0 and 1 go out under this sub-tile's last two steps and
    // its step 0 is formed under the last (behind the workgroup's last sub-tile the other buffer holds zeros or stale data and
    // what is formed from it is dropped)
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    rd(nxt, IC<0>{}, rawA); xf(rawB, opB); stage(nxt, IC<6>{}, live2);
    mfma16(opA);
    WGW_STEP_END();
    bsum += (double)bs;   // (step 0's share is added when it is formed, under the last step)
    bs = 0.f;
    rd(nxt, IC<1>{}, rawB); xf(rawA, opA); stage(nxt, IC<7>{}, live2);
    mfma16(opB);
    WGW_STEP_END();
  }

  // ---- G^T dU G: y and x part in the wave (xi = 3 carries the opposite sign) -> LDS [xi_z][ky*3+kx][c][k]; z part across the waves ----
  asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
  __syncthreads();   // (the last step formed operands from the other buffer)
  float* xl = lds + wave * 9 * 1024;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float m[3][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float u0 = wgw_acc_rd(acc[0][b][r]), u1 = wgw_acc_rd(acc[1][b][r]), u2 = wgw_acc_rd(acc[2][b][r]),
                  u3 = wgw_acc_rd(acc[3][b][r]);
      const float hs = 0.5f * (u1 + u2), hd = 0.5f * (u1 - u2);
      m[0][b] = u0 + hs;
      m[1][b] = hd;
      m[2][b] = hs - u3;
    }
    const int crow = 8 * (r >> 2) + 4 * hh + (r & 3);   // = wg_acc_row(r, hh), which compiles to another schedule here
    float* o = xl + crow * 32 + ch;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const float hs = 0.5f * (m[ky][1] + m[ky][2]), hd = 0.5f * (m[ky][1] - m[ky][2]);
      o[(ky * 3 + 0) * 1024] = m[ky][0] + hs;
      o[(ky * 3 + 1) * 1024] = hd;
      o[(ky * 3 + 2) * 1024] = hs - m[ky][3];
    }
  }
  __syncthreads();
  // taps (kz, ky, kx): kz 0: L0 + .5 L1 + .5 L2 | kz 1: .5 L1 - .5 L2 | kz 2: .5 L1 + .5 L2 - L3   (L3 accumulated with +q1)
  float* out = p.partial + wg_partial_base(pct, qct, 27);
  for (int e = tid; e < 9 * 1024; e += WGW_THREADS) {
    const float l0 = lds[0 * 9 * 1024 + e], l1 = lds[1 * 9 * 1024 + e], l2 = lds[2 * 9 * 1024 + e], l3 = lds[3 * 9 * 1024 + e];
    const float hs = 0.5f * (l1 + l2), hd = 0.5f * (l1 - l2);
    out[0 * 9 * 1024 + e] = l0 + hs;   // e = (ky*3 + kx) * 1024 + c * 32 + k
    out[1 * 9 * 1024 + e] = hd;
    out[2 * 9 * 1024 + e] = hs - l3;
  }
  if (bias) {
    const double o = __shfl_xor(bsum, 32, 64);   // the two patch parities of the wave
    if (lane < 32) p.partial_b[((long)blockIdx.x * gridDim.z + qct) * 32 + ch] = bsum + o;
  }
}

int bts_wgw_launch_(const WgChoice& ch, const WgradParams& p, hipStream_t stream) {
  static bool attr_done = false;
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(wgw_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
    attr_done = true;
  }
  const bool prof = bts_prof_on();
  if (prof) bts_prof_begin(ch.sym, ch.flops, stream);
  (void)hipGetLastError();
  hipLaunchKernelGGL(wgw_kernel, dim3(ch.nsp, ch.npct, ch.nqct), dim3(WGW_THREADS), (size_t)2 * WGW_BUF * sizeof(float), stream, p);
  if (prof) bts_prof_end(stream);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
