// g++ build of the renderer with RR_OPT_STREAK_LEAN, for tests/test_streak_lean_host.py: hostemu.cpp as it is -- every entry
// point, under its own name, in a library of its own -- with plan_drop's defaulted `lean` argument (rr_device.h
// RR_PLAN_LEAN_DEFAULT) reading the mode set here.  0 is libhostemu.so's arithmetic.
static int rr_lean_emu_mode = 0;
#define RR_PLAN_LEAN_DEFAULT rr_lean_emu_mode
#include "hostemu.cpp"

extern "C" void emu_set_streak_lean(int lean) { rr_lean_emu_mode = lean; }
