// kernels_shade_motion.hip — k_shade's three builds for a moving camera whose differentials are read (MOT, kernels_shade.hip),
// in a translation unit of their own so that they compile beside the others: the kernel template and its helpers come from
// kernels_shade.hip, which under IILE_SHADE_MOTION_TU leaves out its other kernels and launchers and defines launch_shade_motion.
#define IILE_SHADE_MOTION_TU 1
#include "kernels_shade.hip"
