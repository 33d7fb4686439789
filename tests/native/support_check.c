/* support_check.c -- drives the HOST side of support (strainer2_amd/csrc/sk_host_support.c: the samples, the merge of a replayed run's
 * emission lists across the strains of a group, the device's numbers added beside them, and the two formatters) as a stand-alone
 * program, so that it can run under AddressSanitizer + UBSan.  It includes that file and nothing else of the library.  Built and run by
 * tests/test_support_model_host.py: argv[1] is a script, argv[2] receives every strain's .coverage_support ("== <strain>" in front of
 * each), argv[3] the pairs file.  The script's lines:
 *   N <strains> <group>            first line
 *   S <name>                       a strain's name, <strains> of them
 *   T <path>                       the next target
 *   R                              a replayed run begins: one empty list per strain
 *   E <strain> <pair> <lines> <parts>   an emission of the run (pairs ascending within a strain)
 *   M                              the run is merged and its lists are freed
 *   D <first> <n> <3n + 2nn numbers>    what the device returned for n strains: pairs, lines, both, shared, lines_a */
#include "../../strainer2_amd/csrc/sk_host_support.c"

int main(int argc, char **argv)
{
    FILE *in, *f;
    sks_acc *a = NULL;
    sks_list *lists = NULL;
    char **names = NULL, line[1 << 16];
    uint32_t ns = 0, group = 0, nn = 0, s;
    int sample = -1, bad = 0;
    if (argc != 4 || !(in = fopen(argv[1], "r"))) { fprintf(stderr, "usage: support_check script support.out pairs.out\n"); return 2; }
    while (!bad && fgets(line, sizeof line, in)) {
        line[strcspn(line, "\n")] = 0;
        if (line[0] == 'N') {
            if (sscanf(line + 1, "%u %u", &ns, &group) != 2 || !(a = sks_create(ns, group))) bad = 1;
            else { names = (char **)calloc(ns, sizeof *names); lists = (sks_list *)calloc(ns, sizeof *lists); bad = !names || !lists; }
        } else if (!a) bad = 1;
        else if (line[0] == 'S') { if (nn < ns) names[nn++] = strdup(line + 2); else bad = 1; }
        else if (line[0] == 'T') bad = (sample = sks_sample(a, line + 2)) < 0;
        else if (line[0] == 'R') { for (s = 0; s < ns; s++) if (lists[s].n) bad = 1; }
        else if (line[0] == 'E') {
            uint32_t st, pr, ln, pa;
            if (sscanf(line + 1, "%u %u %u %u", &st, &pr, &ln, &pa) != 4 || st >= ns || sks_list_push(&lists[st], pr, ln, pa)) bad = 1;
        } else if (line[0] == 'M') {
            bad = sample < 0 || sks_merge(a, (uint32_t)sample, lists);
            for (s = 0; s < ns; s++) sks_list_free(&lists[s]);
        } else if (line[0] == 'D') {
            uint32_t first, n, k;
            int used = 0, step;
            uint64_t *v;
            if (sscanf(line + 1, "%u %u%n", &first, &n, &used) != 2 || !n || n > ns) { bad = 1; break; }
            v = (uint64_t *)calloc((size_t)3 * n + (size_t)2 * n * n, sizeof *v);
            for (k = 0; v && k < 3 * n + 2 * n * n; k++) {
                unsigned long long x;
                if (sscanf(line + 1 + used, "%llu%n", &x, &step) != 1) { bad = 1; break; }
                v[k] = x; used += step;
            }
            if (!v || sample < 0) bad = 1;
            if (!bad) bad = sks_add_device(a, (uint32_t)sample, first, n, v, v + n, v + 2 * n, v + 3 * n, v + 3 * n + (size_t)n * n) != 0;
            free(v);
        } else if (line[0]) bad = 1;
    }
    fclose(in);
    if (!bad && nn != ns) bad = 1;
    if (!bad && (f = fopen(argv[2], "w"))) {
        for (s = 0; s < ns && !bad; s++) { fprintf(f, "== %s\n", names[s]); bad = sks_write_support(a, s, f) != 0; }
        if (fclose(f)) bad = 1;
    } else bad = 1;
    if (!bad && (f = fopen(argv[3], "w"))) {
        bad = sks_write_pairs(a, (const char *const *)names, f) != 0;
        if (fclose(f)) bad = 1;
    } else bad = 1;
    for (s = 0; names && s < ns; s++) free(names[s]);
    for (s = 0; lists && s < ns; s++) sks_list_free(&lists[s]);
    free(names); free(lists);
    sks_destroy(a);
    if (bad) { fprintf(stderr, "support_check: bad script or a call failed\n"); return 1; }
    return 0;
}
