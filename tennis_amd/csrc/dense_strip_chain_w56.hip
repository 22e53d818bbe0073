// the chained dense_strip kernel of the 56 x 56 maps: the block's strip layers in one launch (a translation unit of its own:
// its 5 layer bodies take as long to compile as the per-layer instantiations of the width, and make builds the units in parallel)
#include "dense_strip_impl.h"

int launch_dense_strip_chain_w56(const DenseStripChainArgs &a, hipStream_t s) { return launch_strip_chain<56>(a, s); }
