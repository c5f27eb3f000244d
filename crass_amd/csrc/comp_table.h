// comp_table.h — reverseComplement's table (SeqUtils.cpp:50-59), one definition for host and device code.
//
// A byte b is looked up at b & 127.  Host code uses kCompTable; a .hip that needs the table on the device defines
//     static __constant__ CompTable c_comp = make_comp_table();
// which the compiler fills in: nothing is uploaded.
#pragma once

namespace crass {

struct CompTable { unsigned char v[128]; };

constexpr CompTable make_comp_table()
{
    // IUPAC complement pairs, U->A, everything else maps to itself; entry 96 ('`') holds 64,
    // exactly like the reference table (SeqUtils.cpp:50-59).
    CompTable t{};
    for (int i = 0; i < 128; i++) t.v[i] = (unsigned char)i;
    const char a[] = "ACBDKRSWN", b[] = "TGVHMYSWN";
    for (int i = 0; a[i]; i++) {
        t.v[(int)a[i]] = (unsigned char)b[i];
        t.v[(int)b[i]] = (unsigned char)a[i];
        t.v[(int)a[i] + 32] = (unsigned char)(b[i] + 32);
        t.v[(int)b[i] + 32] = (unsigned char)(a[i] + 32);
    }
    t.v['U'] = 'A';
    t.v['u'] = 'a';
    t.v[96] = 64;
    return t;
}

constexpr CompTable kCompTable = make_comp_table();

} // namespace crass
