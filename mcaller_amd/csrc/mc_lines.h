// mc_lines.h -- the line starts of a text on the device, for a unit other than mc_tables.hip: kp_count (newlines per 16 KB tile),
// kp_scan (exclusive scan, one workgroup), kp_starts (the offsets behind every newline, KpHead.n_lines).  The kernels are those of
// the device parser and are defined once, in mc_devparse.inc; this header includes that file with everything but them left out.
// Like every kernel there they sit in an unnamed namespace: a unit that includes this header gets its own instances.  The five file
// pipelines' units include it through mc_textfeed.h, which launches the three kernels for them (lines_count, lines_starts).
#pragma once
#include "mc_ctx.h"

#define MC_LINES_ONLY
#include "mc_devparse.inc"
#undef MC_LINES_ONLY
