// inputs_main.cpp -- every answer of csrc/tlb_inputs.h, printed: one line "level present family answer" for each mask of present families
// and each family to set, at stream level (the four families a batch has) and at object level (all five).  tests/test_inputs_rule.py builds
// this with AddressSanitizer and UBSan and compares the lines with the two relations written out there.
#include <stdio.h>

#include "../../odr-audioenc_amd/csrc/tlb_inputs.h"

int main()
{
    int lines = 0;
    for (int level = 0; level < TLB_INPUTS_LEVELS; level++) {
        const int families = level == TLB_INPUTS_STREAM ? TLB_IN_SHORT_READS : TLB_IN_COUNT;
        for (unsigned present = 0; present < (1u << families); present++)
            for (int f = 0; f < families; f++, lines++)
                printf("%d %u %d %d\n", level, present, f, tlb_input_may_set((TlbInputLevel)level, (TlbInput)f, present) ? 1 : 0);
    }
    printf("inputs ok: %d answers\n", lines);
    return 0;
}
