// rover_render.hpp -- rendering constants of the rgb_array viewer (viewer_kernels.hip).  DESIGN.md section 11.
//
// Everything here is a RENDERING CHOICE, not part of the rover model: the reference asset's visual meshes are not in
// rover_model.json, so the chassis is a box and the wheels are plain cylinders of the model's contact radius.  The CPU oracle
// (tests/viewer_reference.py) restates these values and tests/test_viewer.py checks that it restates them exactly.
#pragma once

// ---- geometry (Body frame, metres)
#define RR_CHASSIS_CENTER {0.0f, 0.0f, 0.06f}        // box centre
#define RR_CHASSIS_HALF {0.36f, 0.22f, 0.08f}        // box half extents (x, y, z)
#define RR_WHEEL_HALF_WIDTH 0.05f                    // wheel cylinder: radius RV_WHEEL_CONTACT_RADIUS, length 2 x this
#define RR_TARGET_RADIUS 0.12f                       // target sphere: centre = ROVER_TARGET_W + (0, 0, RR_TARGET_Z_OFFSET)
#define RR_TARGET_Z_OFFSET 0.30f

// ---- default lens: Kit's default perspective camera /OmniverseKit_Persp, which ORBIT's viewer renders from (ASSUMPTION: the
// values of that prim as Kit creates it; they are not in the reference checkout).  Horizontal FOV = 2 atan(20.955 / (2 x 18.147562))
// = 60.0 deg; square pixels.
#define RR_FOCAL_LENGTH 18.147562f                   // mm
#define RR_HORIZONTAL_APERTURE 20.955f               // mm
#define RR_NEAR_CLIP 0.01f                           // m
#define RR_FAR_CLIP 1000000.0f                       // m

// ---- shading: rgb = round(255 clamp(albedo (K_A + K_D max(0, n . l)), 0, 1)), l = unit vector hit -> RR_LIGHT_POS
#define RR_LIGHT_POS {0.0f, -180.0f, 80.0f}          // the reference's sphere light (rover_env_cfg.py:65)
#define RR_K_AMBIENT 0.35f
#define RR_K_DIFFUSE 0.65f
#define RR_ALBEDO_GROUND {0.62f, 0.52f, 0.40f}
#define RR_ALBEDO_ROCK {0.42f, 0.40f, 0.40f}         // the hit triangle has a corner whose obstacle layer exceeds RR_ROCK_EPS
#define RR_ALBEDO_CHASSIS {0.85f, 0.85f, 0.88f}
#define RR_ALBEDO_WHEEL {0.14f, 0.14f, 0.15f}
#define RR_ALBEDO_TARGET {0.95f, 0.22f, 0.16f}
#define RR_ROCK_EPS 1.0e-3f                          // m, = RV_OBSTACLE_EPS (the contact report's rock test)
// sky: horizon + (zenith - horizon) max(0, d.z), rounded like the shaded colours
#define RR_SKY_HORIZON {0.80f, 0.85f, 0.92f}
#define RR_SKY_ZENITH {0.36f, 0.56f, 0.86f}

// ---- object ids (the object_id image): sky, ground, rock, then 8 per env: chassis, wheels FL FR CL CR RL RR, target
#define RR_ID_SKY 0
#define RR_ID_GROUND 1
#define RR_ID_ROCK 2
#define RR_ID_ENV0 3
#define RR_IDS_PER_ENV 8
