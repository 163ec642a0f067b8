// lift_render.hpp -- constants of the rgb_array viewer of FrankaCubeLift-v0 (lift_viewer_kernels.hip).  DESIGN.md section 29.
//
// Two kinds of values.  (1) The viewer's COPIES of the model data it draws from (lift_kernels.hip owns the originals and stays
// untouched): rover_lift_viewer_constants returns them and tests/test_lift_viewer.py checks them entry by entry against
// rover_lift_model_constants.  (2) RENDERING CHOICES, not part of the model: the reference asset's visual meshes are not in the
// checkout, so the arm is a chain of capsules, the hand and fingers are boxes and the table is a slab.  The CPU reference
// (tests/lift_viewer_reference.py) restates (2) and tests/test_lift_viewer.py checks that it restates them exactly.
// Lens, light, shading weights and sky are rover_render.hpp's.
#pragma once

// ---- (1) model data: modified DH (Craig) of the Panda, kind = 0 / +1 / -1 for alpha = 0 / +pi/2 / -pi/2
#define LR_KIND {0, -1, 1, 1, -1, 1, 1}
#define LR_DH_A {0.0f, 0.0f, 0.0f, 0.0825f, -0.0825f, 0.0f, 0.088f}
#define LR_DH_D {0.333f, 0.0f, 0.316f, 0.0f, 0.384f, 0.0f, 0.0f}
#define LR_FLANGE_D 0.107f                           // K_FLANGE_D
#define LR_CUBE_HALF 0.02f                           // K_CUBE_HALF
#define LR_PAD_HALF_X 0.010f                         // K_PAD_HALF_X
#define LR_PAD_HALF_Z 0.009f                         // K_PAD_HALF_Z

// ---- (2) geometry (metres)
#define LR_ARM_RADIUS 0.055f                         // the one radius of the eight arm capsules
#define LR_TABLE_CENTER {0.35f, 0.0f, -0.03f}        // slab under z = 0, env frame: x -0.3 .. 1.0, y -0.85 .. 0.85 covers the cube's
#define LR_TABLE_HALF {0.65f, 0.85f, 0.03f}          // spawn range (x 0.4 .. 0.6, y -0.25 .. 0.25) and the command range (0.3 .. 0.7)
#define LR_HAND_CENTER_Z 0.033f                      // hand box: centre = flange + z_hand x this, half extents in the hand frame
#define LR_HAND_HALF {0.0315f, 0.102f, 0.033f}
#define LR_FINGER_THICKNESS 0.012f                   // finger box: from the pad plane outwards along +-y_hand
#define LR_FINGER_LENGTH 0.030f                      // finger box: this far behind the pad (-z_hand); the pad itself is 2 K_PAD_HALF_Z
#define LR_GOAL_RADIUS 0.03f
#define LR_GROUND_Z -1.05f                           // the reference's ground plane (manipulation_env_cfg.py:88)

// ---- (2) albedos
#define LR_ALBEDO_GROUND {0.55f, 0.55f, 0.56f}
#define LR_ALBEDO_TABLE {0.60f, 0.45f, 0.30f}
#define LR_ALBEDO_ARM {0.90f, 0.90f, 0.92f}
#define LR_ALBEDO_HAND {0.80f, 0.80f, 0.84f}
#define LR_ALBEDO_FINGER {0.20f, 0.20f, 0.22f}
#define LR_ALBEDO_CUBE {0.20f, 0.45f, 0.85f}
#define LR_ALBEDO_GOAL {0.95f, 0.22f, 0.16f}

// ---- object ids: sky, ground, then 16 per env: table, arm segments 1..8, hand, finger 0, finger 1, cube, goal (14, 15 unused)
#define LR_ID_SKY 0
#define LR_ID_GROUND 1
#define LR_ID_ENV0 2
#define LR_IDS_PER_ENV 16
#define LR_K_TABLE 0
#define LR_K_ARM0 1
#define LR_K_HAND 9
#define LR_K_FINGER0 10
#define LR_K_CUBE 12
#define LR_K_GOAL 13

// ---- traversal (not visible in the image): every env whose bounds stay inside this z slab and inside the 3 x 3 lattice cells
// around its own is found by the rays' lattice walk; the others go to the overflow list every ray tests
#define LR_SLAB_Z_LO -0.5f
#define LR_SLAB_Z_HI 2.5f
#define LR_CELL_MARGIN 1.0e-3f                       // cells: bounds must stay this far inside the 3 x 3 neighbourhood
#define LR_BOUND_MAX 1.0e6f                          // m: a larger bounding radius is stored as +inf (the cull passes every ray)
