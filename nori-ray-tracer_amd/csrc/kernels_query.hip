// kernels_query.hip -- translation unit 4 of kernels.hip: k_surface,
// k_camera_rays and their launchers (see the NORI_TU note there).
#define NORI_TU 4
#include "kernels.hip"
