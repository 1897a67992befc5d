// kernels_features.hip -- translation unit 3 of kernels.hip: k_features and
// launch_features (see the NORI_TU note there).
#define NORI_TU 3
#include "kernels.hip"
