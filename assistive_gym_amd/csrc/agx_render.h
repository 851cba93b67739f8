// agx_render.h -- what agx_api.hip hands to the ray caster of csrc/agx_render.hip (agx_camera_set / agx_render, include/agx.h), and the one
// colour table of the camera.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// colour per collider tag (AGX_TAG_*, include/agx_blob.h: 1 robot ... 9 bed; 0 = a collider without a tag), then the water particles of the
// drinking scenes and the background.  agx_camera_colours copies it out, so that Python and the tests read this table and keep no copy.
#define AGX_COLOUR_WATER 10
#define AGX_COLOUR_BACKGROUND 11
#define AGX_COLOUR_COUNT 12
static const float AGX_COLOURS[AGX_COLOUR_COUNT][3] = {
  {0.50f, 0.50f, 0.50f},      // untagged
  {0.75f, 0.75f, 0.78f},      // robot
  {0.85f, 0.85f, 0.90f},      // tool
  {0.96f, 0.76f, 0.62f},      // human
  {0.24f, 0.71f, 0.29f},      // food
  {1.00f, 1.00f, 1.00f},      // bowl
  {0.60f, 0.45f, 0.30f},      // table
  {0.85f, 0.85f, 0.85f},      // ground plane
  {0.20f, 0.20f, 0.22f},      // wheelchair
  {0.90f, 0.90f, 0.85f},      // bed
  {0.25f, 0.50f, 1.00f},      // water
  {0.80f, 0.90f, 1.00f},      // background (the reference's GUI clear colour)
};
// the garment of a dressing scene (agx_camera_garment): the gown's own colour, dressing.py:153 rgbaColor = [139, 195, 74] / 256, drawn opaque.
// Not a row of AGX_COLOURS: agx_camera_colours keeps its 12 x 3 layout; agx_camera_garment_colour copies this one out.
// On the device it is the row behind the table's last (AGX_COLOUR_GARMENT of agx_render_args::colours).
static const float AGX_GARMENT_COLOUR[3] = {139.f / 256.f, 195.f / 256.f, 74.f / 256.f};
#define AGX_COLOUR_GARMENT AGX_COLOUR_COUNT

// image tile of one workgroup (one wavefront): 16 pixels of 4 rows, so that a row of the tile is one 64-byte piece of an image row
#define AGX_RENDER_TW 16
#define AGX_RENDER_TH 4
// most colliders + particles a tile's list holds (LDS); agx_camera_set refuses larger scenes
#define AGX_RENDER_LIST 1024

// per collider, built on the host by agx_camera_set: where its face planes are (hulls; count 0 = sphere / capsule core), which genders see it
// (bit 0 male, bit 1 female), and the radius about its AGX_C_AABB_C of a sphere that holds everything drawn of it
struct agx_render_coll { int plane0, nplane, genders; float bound; };

struct agx_render_args {
  const uint32_t* blob; const float* state; int sw;
  const float* frames;                       // [n_envs][ncoll][12]: position, rotation (row-major) of every collider's body, from the frames kernel
  const agx_render_coll* coll;               // [ncoll]
  const float4* planes;                      // outward unit normal, offset grown by the collider's radius and taken relative to AGX_C_AABB_C
  const float* water; int cloth_words, npart; float part_radius;      // water particles [n_envs][cloth_words] (positions first), or null / 0
  const float* colours;                      // AGX_COLOURS on the device, then AGX_GARMENT_COLOUR as row AGX_COLOUR_GARMENT
  float eye[3], right[3], up[3], fwd[3];     // world: a pixel's ray is eye + t (x right + y up + fwd), so t is the depth along fwd
  float tx, ty;                              // aspect tan(fov / 2), tan(fov / 2)
  int width, height; float near, far;
  float light[3], ambient, diffuse;          // unit vector towards the light
  int env0;
  float* depth; int* seg; uint32_t* rgba;    // [count][height][width], each may be null
  // the garment (agx_camera_garment; read by the garment kernel only): the triangle table of csrc/agx_garment.h as {a, b, c, 0}[ntri], and the
  // garments [n_envs][cloth_words], of which the first [nodes][3] floats of a record are the node positions
  const int4* tris; int ntri; const float* garment;
};

// garment: the garment kernel follows the rigid caster on the same stream (A.tris, A.garment, A.cloth_words set; A.depth and A.seg not null)
void agx_launch_render(hipStream_t st, const agx_render_args& A, int count, bool garment);
