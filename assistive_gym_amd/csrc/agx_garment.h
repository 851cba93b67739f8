// agx_garment.h -- host side of the camera's garment kernel (csrc/agx_render.hip): the triangle table of a dressing scene's garment, built from the
// model blob alone when agx_camera_garment first switches the garment on (and by agx_garment_faces).  Plain C++ without HIP, so that g++ compiles
// it alone (tests/garment_faces/).  The rule (include/agx.h): walk the nodes a = 0 .. NN-1 in order and each node's incident-face entries (j, k)
// (AGX_CL_OFF_FACE, from AGX_CL_OFF_NODE) in order; keep (a, j, k) when a < j and a < k.  A face has three rotated entries, so it is kept once,
// in its winding; face f is the f-th kept triple.  The section is not trusted: everything read from it is checked against the blob's size first.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "../../include/agx_blob.h"

namespace agxgarment {

// tris: [faces][3] node indices, empty for a blob without a cloth section or with a particle section (the water: no faces, not a garment).
// Returns 0, or -1 with *err naming what is wrong with the section (tris is then empty).
inline int garment_faces(const int32_t* w, size_t nwords, std::vector<int>& tris, const char** err) {
  tris.clear();
  auto bad = [&](const char* what) { tris.clear(); if (err) *err = what; return -1; };
  if (!w || nwords < (size_t)AGX_H_COUNT) return bad("the blob is shorter than its header");
  const int64_t oc = w[AGX_H_OFF_CLOTH];
  if (oc == 0) return 0;
  if (oc < (int64_t)AGX_H_COUNT || (uint64_t)oc + AGX_CL_HDR > nwords) return bad("the cloth section's header lies outside the blob");
  const int32_t* cl = w + oc;
  const int64_t sec = (int64_t)nwords - oc;      // words from the section's start to the blob's end: what an offset of the section may reach
  if (cl[AGX_CL_PARTICLES] != 0) return 0;
  const int64_t nn = cl[AGX_CL_NN], o_node = cl[AGX_CL_OFF_NODE], o_face = cl[AGX_CL_OFF_FACE];
  if (nn < 0 || nn > 65535) return bad("the node count is outside 0..65535");      // an entry packs two 16-bit node indices
  if (o_node < AGX_CL_HDR || o_node + 2 * (nn + 1) > sec) return bad("the node table lies outside the section");
  const int32_t* node = cl + o_node;      // {first incident-face entry, area}[NN + 1]
  const int64_t entries = node[2 * nn];
  if (entries < 0 || entries % 3 != 0) return bad("the entry count is not a multiple of 3");
  if (o_face < AGX_CL_HDR || o_face + entries > sec) return bad("the face entries lie outside the section");
  const int32_t* face = cl + o_face;
  if (node[0] != 0) return bad("the first node's entries do not start at 0");
  tris.reserve((size_t)entries);
  for (int64_t a = 0; a < nn; a++) {
    const int64_t e0 = node[2 * a], e1 = node[2 * (a + 1)];
    if (e0 > e1 || e1 > entries) return bad("a node's entry range is not inside the entries");
    for (int64_t e = e0; e < e1; e++) {
      const int j = face[e] & 0xffff, k = (int)(((uint32_t)face[e]) >> 16);
      if (j >= nn || k >= nn) return bad("an entry names a node index >= NN");
      if (a < j && a < k) { tris.push_back((int)a); tris.push_back(j); tris.push_back(k); }
    }
  }
  if ((int64_t)tris.size() != entries) return bad("the entries are not three rotations of every face");      // 3 ints per kept face = 3 entries per face
  return 0;
}

}  // namespace agxgarment
