// version_diff_driver.cpp -- stand-alone driver of longtail_amd/csrc/version_diff.h (over restore_parse.h) for
// tests/test_version_diff_san.py: built with -fsanitize=address,undefined and run as a program.  It includes the header and nothing else
// of the library.
//   version_diff_driver SOURCE TARGET
// Both files hold VALID serialized VersionIndexes.  Every blob is offered as a heap copy of exactly its bytes (a read past them is the
// sanitizer's to report):
//   both blobs whole                                    -> 0, the six lists printed one per line
//   every proper prefix of either, the other whole      -> EBADF
// and prints "ok <cases>" last; the first wrong answer is printed and the exit status is 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../longtail_amd/csrc/version_diff.h"

static std::vector<uint8_t> read_file(const char* path)
{
    std::vector<uint8_t> blob;
    FILE* f = fopen(path, "rb");
    if (!f)
        exit(2);
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;)
        blob.insert(blob.end(), buf, buf + n);
    fclose(f);
    return blob;
}

static int diff(const std::vector<uint8_t>& a, size_t na, const std::vector<uint8_t>& b, size_t nb, version_diff::Lists* out)
{
    uint8_t* ca = (uint8_t*)malloc(na ? na : 1);
    uint8_t* cb = (uint8_t*)malloc(nb ? nb : 1);
    if (na)
        memcpy(ca, a.data(), na);
    if (nb)
        memcpy(cb, b.data(), nb);
    const int err = version_diff::diff(ca, na, cb, nb, out);
    free(ca);
    free(cb);
    return err;
}

static void print(const char* name, const std::vector<uint32_t>& v)
{
    printf("%s", name);
    for (const uint32_t x : v)
        printf(" %u", x);
    printf("\n");
}

int main(int argc, char** argv)
{
    if (argc != 3)
        return 2;
    const std::vector<uint8_t> a = read_file(argv[1]), b = read_file(argv[2]);
    version_diff::Lists whole;
    int err = diff(a, a.size(), b, b.size(), &whole);
    if (err)
    {
        printf("FAIL the valid blobs: errno %d\n", err);
        return 1;
    }
    print("source_removed", whole.source_removed);
    print("target_added", whole.target_added);
    print("source_content", whole.source_content);
    print("target_content", whole.target_content);
    print("source_permissions", whole.source_permissions);
    print("target_permissions", whole.target_permissions);
    unsigned long long cases = 1;
    for (int side = 0; side < 2; ++side)
        for (size_t n = 0; n < (side ? b.size() : a.size()); ++n, ++cases)
        {
            version_diff::Lists d;
            err = side ? diff(a, a.size(), b, n, &d) : diff(a, n, b, b.size(), &d);
            if (err != EBADF)
            {
                printf("FAIL prefix %zu of %s: errno %d, expected %d\n", n, side ? "the target" : "the source", err, EBADF);
                return 1;
            }
        }
    printf("ok %llu\n", cases);
    return 0;
}
