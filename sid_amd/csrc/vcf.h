// vcf.h — the VCF record of a site (sid.h Conventions, "VCF"), shared by the
// host formatter (emit.cpp, sid_format_vcf) and the device stage
// (textpath.hip, sid_vcf_len_kernel / sid_vcf_put_kernel): which alleles a
// record names, how long its fixed part is, and its bytes around the chrom,
// the position and the two confidence texts.
//
//   CHROM \t POS \t . \t REF \t ALT \t . \t . \t DP=d;HOM=h;HET=e \t GT \t g \n
//
// A record is a pure function of its CSV record (chrom, pos, the two gt bytes,
// the two %g texts), the site's reference class and its depth.
#pragma once

#include <stdint.h>

// (host-only translation units compiled as plain C++ have no __host__ / __device__)
#ifdef __HIP__
#define SID_VCF_HD __host__ __device__
#else
#define SID_VCF_HD
#endif

// the header's lines between "##source=..." and "##sidConfType=..." / behind it
#define SID_VCF_HEAD_INFO                                                                                       \
    "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Counted bases A+C+G+T of the site's profile\">\n"        \
    "##INFO=<ID=HOM,Number=1,Type=Float,Description=\"Confidence of the homozygous call (hom_conf)\">\n"        \
    "##INFO=<ID=HET,Number=1,Type=Float,Description=\"Confidence of the heterozygous call (het_conf)\">\n"
#define SID_VCF_HEAD_TAIL                                                   \
    "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"      \
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"

// A record's bytes besides its chrom, its position's digits, ALT, DP's digits
// and the two confidences: \t \t.\t R \t (ALT) \t.\t.\tDP= (d) ;HOM= (h) ;HET=
// (e) \tGT\t g \n = 1 + 3 + 1 + 1 + 8 + 5 + 5 + 4 + 3 + 1.
#define SID_VCF_FIXED 32
// ... and the most a record holds besides its chrom: an 11-byte position, ALT
// "X,Y", a six-digit depth (4 x 65535) and two 13-byte %g texts
#define SID_VCF_REC_MAX (SID_VCF_FIXED + 11 + 3 + 6 + 13 + 13)

struct sid_vcf_gt {
    char ref;      // 'A', 'C', 'G', 'T' or 'N'
    char alt[2];   // the ALT alleles in order
    int nalt;      // 0 .. 2 (0: ALT is ".")
    char g[2];     // the two allele numbers, the smaller first ('.': no call)
};

// refcls: 0 .. 3 = A, C, G, T (either case in the text), anything else = N; x,
// y: the CSV record's two gt bytes; depth: A + C + G + T of the profile
SID_VCF_HD inline sid_vcf_gt sid_vcf_call(uint32_t refcls, char x, char y, uint32_t depth)
{
    sid_vcf_gt v;
    v.ref = refcls < 4u ? (char)((0x54474341u >> (8u * refcls)) & 0xFFu) : 'N';
    v.alt[0] = v.alt[1] = 0;
    v.nalt = 0;
    v.g[0] = v.g[1] = '.';
    if (depth == 0) return v;   // no counted base: -m local's "hom,TT" placeholder names nothing
    if (x != v.ref) v.alt[v.nalt++] = x;
    if (y != v.ref && y != x) v.alt[v.nalt++] = y;
    const int ax = x == v.ref ? 0 : 1;   // (x, when it is no REF, is ALT 1)
    const int ay = y == v.ref ? 0 : y == v.alt[0] ? 1 : 2;
    v.g[0] = (char)('0' + (ax < ay ? ax : ay));
    v.g[1] = (char)('0' + (ax < ay ? ay : ax));
    return v;
}

SID_VCF_HD inline int sid_vcf_u32_len(uint32_t v)
{
    int n = 1;
    for (uint32_t p = 10; n < 10 && v >= p; p *= 10) ++n;
    return n;
}

// the record's bytes besides its chrom, its position's digits and the two confidence texts
SID_VCF_HD inline int sid_vcf_mid_len(const sid_vcf_gt& v, uint32_t depth)
{
    return SID_VCF_FIXED + (v.nalt == 2 ? 3 : 1) + sid_vcf_u32_len(depth);
}

// "\t.\tR\tALT\t.\t.\tDP=d;HOM=" through put(k, byte) from byte n on; returns the next byte's index
template <class Put>
SID_VCF_HD inline uint32_t sid_vcf_put_a(uint32_t n, const sid_vcf_gt& v, uint32_t depth, Put put)
{
    put(n++, '\t'), put(n++, '.'), put(n++, '\t');
    put(n++, (uint32_t)(uint8_t)v.ref);
    put(n++, '\t');
    if (v.nalt == 0) put(n++, '.');
    else put(n++, (uint32_t)(uint8_t)v.alt[0]);
    if (v.nalt == 2) put(n++, ','), put(n++, (uint32_t)(uint8_t)v.alt[1]);
    put(n++, '\t'), put(n++, '.'), put(n++, '\t'), put(n++, '.'), put(n++, '\t');
    put(n++, 'D'), put(n++, 'P'), put(n++, '=');
    const int dl = sid_vcf_u32_len(depth);
    uint32_t u = depth;
    for (int k = dl - 1; k >= 0; --k) {
        put(n + (uint32_t)k, '0' + u % 10u);
        u /= 10u;
    }
    n += (uint32_t)dl;
    put(n++, ';'), put(n++, 'H'), put(n++, 'O'), put(n++, 'M'), put(n++, '=');
    return n;
}

// ";HET=" between the two confidence texts
template <class Put>
SID_VCF_HD inline uint32_t sid_vcf_put_b(uint32_t n, Put put)
{
    put(n++, ';'), put(n++, 'H'), put(n++, 'E'), put(n++, 'T'), put(n++, '=');
    return n;
}

// "\tGT\tg\n" behind them
template <class Put>
SID_VCF_HD inline uint32_t sid_vcf_put_c(uint32_t n, const sid_vcf_gt& v, Put put)
{
    put(n++, '\t'), put(n++, 'G'), put(n++, 'T'), put(n++, '\t');
    put(n++, (uint32_t)(uint8_t)v.g[0]), put(n++, '/'), put(n++, (uint32_t)(uint8_t)v.g[1]);
    put(n++, '\n');
    return n;
}
