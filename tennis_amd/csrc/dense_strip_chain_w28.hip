// the chained dense_strip kernel of the 28 x 28 maps: the block's strip layers in one launch (a translation unit of its own:
// its 6 layer bodies take as long to compile as the per-layer instantiations of the width, and make builds the units in parallel)
#include "dense_strip_impl.h"

int launch_dense_strip_chain_w28(const DenseStripChainArgs &a, hipStream_t s) { return launch_strip_chain<28>(a, s); }
