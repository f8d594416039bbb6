// The instances of encode_inter_mb / encode_inter_chroma for P pictures with a reference per 8x8
// quadrant (x264 --mixed-refs, H264Params.mixed_refs), in a translation unit of their own: the
// kernels' text is encode_inter.hip's, with what MIVC_INTER_MIXED_UNIT switches on.
#define MIVC_INTER_MIXED_UNIT
#include "encode_inter.hip"
