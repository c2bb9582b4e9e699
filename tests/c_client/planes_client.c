/*
 * planes_client.c -- a plain C99 caller of libtriro_planes.so: no Python, no torch, no C++.
 *
 * One call of every entry of include/triro_planes.h on the two parallel triangles of client.c (z = 0 and z = -1), with
 * answers derived by hand.  TEST-ONLY; built and run by tests/test_planes_cpu.py / tests/test_gpu_planes.py.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "triro_planes.h"

#define CHECK_HIP(x)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #x, hipGetErrorName(e_)); \
            exit(2);                                                                      \
        }                                                                                 \
    } while (0)
#define CHECK_TR(x)                                                                       \
    do {                                                                                  \
        int s_ = (x);                                                                     \
        if (s_ != TR_OK) {                                                                \
            fprintf(stderr, "%s:%d: %s -> %d (%s)\n", __FILE__, __LINE__, #x, s_, tr_last_error()); \
            exit(3);                                                                      \
        }                                                                                 \
    } while (0)
#define EXPECT(c)                                                                         \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            fprintf(stderr, "%s:%d: expectation failed: %s\n", __FILE__, __LINE__, #c);   \
            exit(4);                                                                      \
        }                                                                                 \
    } while (0)

static void *to_device(const void *h, size_t bytes) {
    void *d = NULL;
    CHECK_HIP(hipMalloc(&d, bytes ? bytes : 4));
    if (bytes) CHECK_HIP(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    return d;
}
/* every output is born full of a pattern no answer has: 0xa5 bytes (an any byte is 0 / 1, a count or a face >= 0), 0xff for
 * the floats (a NaN) */
static void *device_poison(size_t bytes, int value) {
    void *d = NULL;
    CHECK_HIP(hipMalloc(&d, bytes ? bytes : 4));
    CHECK_HIP(hipMemset(d, value, bytes ? bytes : 4));
    return d;
}
static void to_host(void *h, const void *d, size_t bytes) { CHECK_HIP(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost)); }

int main(void) {
    const float verts[18] = {0.5f, -0.5f, 0.f, 0.f, 0.5f, 0.f, -0.5f, -0.5f, 0.f,
                             0.5f, -0.5f, -1.f, 0.f, 0.5f, -1.f, -0.5f, -0.5f, -1.f};
    const int32_t faces[6] = {0, 1, 2, 3, 4, 5};
    /* the plane x = 0 cuts both triangles; z = 0 holds the first one (met, not cut); z = -0.5 lies between them; the last
     * normal is zero: an invalid plane */
    const float origins[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, -0.5f, 0.f, 0.f, 0.f};
    const float normals[12] = {2.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    const int32_t keys[7] = {5, -3, 9, 7, 7, -8, 1}, key_count[2] = {3, 3};
    const int64_t key_off[2] = {0, 4};
    float *d_v, *d_o, *d_n, *d_seg;
    int32_t *d_f, *d_cnt, *d_face, *d_keys, *d_kc;
    int64_t *d_off, *d_total, *d_koff, total = -1;
    uint8_t *d_any;
    tr_bvh *bvh = NULL;
    uint8_t any[4];
    int32_t cnt[4], face[2], sorted[7];
    int64_t off[4];
    float seg[12];
    int device = 0, k;

    EXPECT(tr_planes_abi_version() == TR_PLANES_ABI_VERSION);
    EXPECT(tr_planes_frontier_capacity() >= 64);
    CHECK_TR(tr_init(-1));
    CHECK_HIP(hipGetDevice(&device));
    d_v = (float *)to_device(verts, sizeof verts);
    d_f = (int32_t *)to_device(faces, sizeof faces);
    d_o = (float *)to_device(origins, sizeof origins);
    d_n = (float *)to_device(normals, sizeof normals);
    CHECK_TR(tr_bvh_build(d_v, 6, d_f, 2, NULL, &bvh));

    d_any = (uint8_t *)device_poison(4, 0xa5);
    d_cnt = (int32_t *)device_poison(16, 0xa5);
    d_off = (int64_t *)device_poison(32, 0xa5);
    d_total = (int64_t *)device_poison(8, 0xa5);

    /* faces met */
    CHECK_TR(tr_planes_any(bvh, d_o, d_n, 4, d_any, 0, 0, NULL));
    CHECK_TR(tr_planes_count(bvh, d_o, d_n, 4, d_cnt, 0, 1, NULL));
    CHECK_HIP(hipDeviceSynchronize());
    to_host(any, d_any, 4);
    to_host(cnt, d_cnt, 16);
    EXPECT(any[0] == 1 && any[1] == 1 && any[2] == 0 && any[3] == 0);
    EXPECT(cnt[0] == 2 && cnt[1] == 1 && cnt[2] == 0 && cnt[3] == 0);

    /* faces cut: count, scan, fill with segments */
    CHECK_HIP(hipMemset(d_any, 0xa5, 4));
    CHECK_HIP(hipMemset(d_cnt, 0xa5, 16));
    CHECK_TR(tr_planes_any(bvh, d_o, d_n, 4, d_any, 1, 0, NULL));
    CHECK_TR(tr_planes_count(bvh, d_o, d_n, 4, d_cnt, 1, 0, NULL));
    CHECK_TR(tr_hits_scan(d_cnt, 4, INT32_MAX, d_off, d_total, &total, NULL));
    to_host(any, d_any, 4);
    to_host(cnt, d_cnt, 16);
    to_host(off, d_off, 32);
    EXPECT(any[0] == 1 && any[1] == 0 && any[2] == 0 && any[3] == 0);
    EXPECT(cnt[0] == 2 && cnt[1] == 0 && cnt[2] == 0 && cnt[3] == 0);
    EXPECT(total == 2 && off[0] == 0 && off[1] == 2 && off[2] == 2 && off[3] == 2);
    d_face = (int32_t *)device_poison(8, 0xa5);
    d_seg = (float *)device_poison(48, 0xff);
    CHECK_TR(tr_planes_fill(bvh, d_o, d_n, 4, d_cnt, d_off, total, d_face, d_seg, 1, 0, NULL));
    CHECK_HIP(hipDeviceSynchronize());
    to_host(face, d_face, 8);
    to_host(seg, d_seg, 48);
    EXPECT(face[0] == 0 && face[1] == 1);
    /* vertex 0 is positive, vertex 1 lies in the plane, vertex 2 is negative: the walk enters the positive arc on the edge
     * 2 -> 0, at its middle, and leaves it at vertex 1 */
    for (k = 0; k < 2; k++) {
        const float z = k ? -1.f : 0.f;
        EXPECT(seg[6 * k] == 0.f && seg[6 * k + 1] == -0.5f && seg[6 * k + 2] == z);
        EXPECT(seg[6 * k + 3] == 0.f && seg[6 * k + 4] == 0.5f && seg[6 * k + 5] == z);
    }
    /* the lists of the faces met, without segments; segments of faces that are only met are refused */
    CHECK_TR(tr_planes_count(bvh, d_o, d_n, 4, d_cnt, 0, 0, NULL));
    CHECK_TR(tr_hits_scan(d_cnt, 4, INT32_MAX, d_off, d_total, &total, NULL));
    EXPECT(total == 3);
    EXPECT(tr_planes_fill(bvh, d_o, d_n, 4, d_cnt, d_off, total, d_face, d_seg, 0, 0, NULL) == TR_ERR_INVALID_ARG);
    EXPECT(tr_planes_any(bvh, d_o, d_n, 4, d_any, 2, 0, NULL) == TR_ERR_INVALID_ARG);

    /* the ordering pass alone: two segments of three keys, the word between them and the tail untouched */
    d_keys = (int32_t *)to_device(keys, sizeof keys);
    d_kc = (int32_t *)to_device(key_count, sizeof key_count);
    d_koff = (int64_t *)to_device(key_off, sizeof key_off);
    CHECK_TR(tr_planes_order(device, 2, d_kc, d_koff, 7, d_keys, NULL));
    CHECK_HIP(hipDeviceSynchronize());
    to_host(sorted, d_keys, sizeof sorted);
    EXPECT(sorted[0] == -3 && sorted[1] == 5 && sorted[2] == 9 && sorted[3] == 7);
    EXPECT(sorted[4] == -8 && sorted[5] == 1 && sorted[6] == 7);

    CHECK_TR(tr_bvh_destroy(bvh));
    printf("PLANES C CLIENT OK\n");
    return 0;
}
