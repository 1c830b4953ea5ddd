// The per-box arithmetic of the Noise2Void blind-spot masker (n2v.hip; biapy_amd/n2v.py states the semantics): the Philox block of a draw, the
// masked voxel of a box, the clipped window around it and the window voxel that replaces it.  Integers only; compiles for the device and for the
// host (scripts/n2v_cpu_check.cpp walks every box of adversarial shapes through n2v_box under ASan / UBSan and asserts every index in range).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define N2V_HD __host__ __device__ __forceinline__
#else
#define N2V_HD inline
#endif

#define N2V_KEY_XOR 0x4E32564Du      /* the key: (seed low ^ this, seed high) */
#define N2V_MAX_BOX 64
#define N2V_MAX_RADIUS 15
#define N2V_MAX_CHANNELS 8
#define N2V_UNIFORM_WITH_CP 0
#define N2V_UNIFORM_WITHOUT_CP 1
#define N2V_IDENTITY 2
#define N2V_NORMAL_ADDITIVE 3

// extents, box edges, boxes per axis (ceil(dim / s)) and radii; an axis of extent 1 has s = 1 and radius 0
struct N2VGeom {
  int Z, Y, X, sz, sy, sx, nz, ny, nx, rz, ry, rx, manip;
};

// Philox4x32-10 with 64-bit products: the same words as philox.h's, on either side
N2V_HD void n2v_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

N2V_HD uint32_t n2v_mulhi(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * (uint64_t)n) >> 32); }

// What box i of (sample b, channel c) does under the counter value (ql, qh): coord = the linear (z, y, x) index of the masked voxel within the
// sample and source = that of the voxel whose INPUT value replaces it (the voxel itself for identity / normal_additive), or -1 and -1 when the
// box masks nothing (a drawn position beyond a ragged edge; a one-voxel window without its centre).  r0, r1: words 0 and 1 of stream 1.
struct N2VPick {
  int64_t coord, source;
  uint32_t r0, r1;
};

N2V_HD N2VPick n2v_box(const N2VGeom& g, uint32_t k0, uint32_t k1, uint32_t ql, uint32_t qh, uint32_t b, uint32_t c, uint32_t i) {
  N2VPick out;
  out.coord = out.source = -1;
  out.r0 = out.r1 = 0;
  const uint32_t w1 = (b << 4) | c;
  uint32_t r[4];
  n2v_philox(i, w1, ql, qh, k0, k1, r);                                  // stream 0: the position
  const int plane = g.ny * g.nx;
  const int iz = (int)i / plane, rem = (int)i - iz * plane, iy = rem / g.nx, ix = rem - iy * g.nx;
  const int pz = iz * g.sz + (int)n2v_mulhi(r[0], (uint32_t)g.sz), py = iy * g.sy + (int)n2v_mulhi(r[1], (uint32_t)g.sy),
            px = ix * g.sx + (int)n2v_mulhi(r[2], (uint32_t)g.sx);
  if (pz >= g.Z || py >= g.Y || px >= g.X) return out;
  const int64_t p = ((int64_t)pz * g.Y + py) * g.X + px;
  n2v_philox(i, w1 | (1u << 28), ql, qh, k0, k1, r);                     // stream 1: the replacement
  out.r0 = r[0]; out.r1 = r[1];
  if (g.manip == N2V_IDENTITY || g.manip == N2V_NORMAL_ADDITIVE) {
    out.coord = out.source = p;
    return out;
  }
  const int z0 = pz - g.rz > 0 ? pz - g.rz : 0, y0 = py - g.ry > 0 ? py - g.ry : 0, x0 = px - g.rx > 0 ? px - g.rx : 0;
  const int z1 = pz + g.rz + 1 < g.Z ? pz + g.rz + 1 : g.Z, y1 = py + g.ry + 1 < g.Y ? py + g.ry + 1 : g.Y, x1 = px + g.rx + 1 < g.X ? px + g.rx + 1 : g.X;
  const int wz = z1 - z0, wy = y1 - y0, wx = x1 - x0;
  const uint32_t n = (uint32_t)(wz * wy * wx);                           // at most 31^3
  const uint32_t cen = (uint32_t)(((pz - z0) * wy + (py - y0)) * wx + (px - x0));
  uint32_t k;
  if (g.manip == N2V_UNIFORM_WITH_CP) {
    k = n2v_mulhi(r[0], n);
  } else {
    if (n == 1) return out;
    k = n2v_mulhi(r[0], n - 1);
    k += k >= cen ? 1u : 0u;
  }
  const int kz = (int)k / (wy * wx), kr = (int)k - kz * (wy * wx), ky = kr / wx, kx = kr - ky * wx;
  out.coord = p;
  out.source = ((int64_t)(z0 + kz) * g.Y + (y0 + ky)) * g.X + (x0 + kx);
  return out;
}
