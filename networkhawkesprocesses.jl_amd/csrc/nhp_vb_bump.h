// The bump allocator every variational driver carves its reserved block with (continuous: nhp_vb_drive.h, discrete:
// disc_vb.hip): what it handed out is compared with the fit's sizing function before any launch, which ties the sizing to
// the carving.  Plain C++, no model of either side.
#pragma once
#include <cstddef>

struct vb_bump {
    double *base, *p;
    explicit vb_bump(double *b) : base(b), p(b) {}
    double *take(size_t n) { double *r = p; p += n; return r; }
    size_t used() const { return (size_t)(p - base); }
};
