/* kmer_scrub_count -- drop-in replacement for the reference program of the same name
 * (src/kmer_scrub_count.c:29-131): same flags (-r -A -B -C -p, and -d -h -u -H accepted), same
 * stdout TSV in the same row order, same progress file, same stderr texts and exit status.
 * Extension: -S <strains file> WITHOUT -r counts many strains over one pass of the lists
 * (skh_kmer_scrub_count_multi_main), and with --scrub .. --detect takes them on through steps 2-3 (and 4); with -r, -S is what
 * the reference makes of it (usage, ignored).
 * Extension: --prevalence[=FILE] [--prevalence-min-count m] [--prevalence-items=FILE] [--scrub-by prevalence] (with -r): in how
 * many items of each list a k-mer occurs, beside the counts.  With -S the file words take a SUFFIX,
 * --prevalence=SUFFIX [--prevalence-items=SUFFIX]: every strain's table goes to <its outfile><SUFFIX>, from the one pass.
 * All of the work happens in libstrainer_kmer.so (host layer in C, scan in HIP on gfx950). */
#include <stdio.h>
#include <string.h>
#include "../../include/strainer_kmer.h"

/* does the command line carry option letter `opt` (as "-S x", "-Sx" or inside a cluster of flags)?  Follows getopt's
 * reading of "A:B:C:r:p:S:Hhud": the value of an option that takes one is not an option, "--" ends the options */
static int has_opt(int argc, char **argv, char opt)
{
    int i;
    for (i = 1; i < argc; i++) {
        const char *a = argv[i];
        if (a[0] != '-' || a[1] == '\0') continue;
        if (!strcmp(a, "--") || !strcmp(a, "--detect")) break;      /* (what follows --detect is strain_detect's command line) */
        if (a[1] == '-') continue;                     /* (--scrub ...: its value is skipped by the program) */
        for (a++; *a; a++) {
            if (*a == opt) return 1;
            if (strchr("ABCrpS", *a)) { if (a[1] == '\0') i++; break; }
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    static char obuf[1 << 20];
    setvbuf(stdout, obuf, _IOFBF, sizeof obuf);
    if (has_opt(argc, argv, 'S') && !has_opt(argc, argv, 'r'))
        return skh_kmer_scrub_count_multi_main(argc, argv, stdout, stderr);
    return skh_kmer_scrub_count_main(argc, argv, stdout, stderr);
}
