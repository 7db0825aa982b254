// TEST-ONLY: writes TlTables::enwindow (512 doubles) and TlTables::enwindow_s (512 doubles) of the PRODUCT's table builder
// (csrc/mp2_host.cpp tl_build_tables -- the one libmp2emu.so and the device path both call) to stdout, raw.  tests/test_fb_fold_emu.py
// links it with csrc/mp2_host.cpp and compares the bits with a numpy restatement.
#include <stdio.h>

#include "../../odr-audioenc_amd/csrc/mp2_host.h"

int main()
{
    static TlTables T;
    tl_build_tables(&T);
    if (fwrite(T.enwindow, sizeof(double), 512, stdout) != 512) return 1;
    if (fwrite(T.enwindow_s, sizeof(double), 512, stdout) != 512) return 1;
    return 0;
}
