/* Preloaded in front of fakehip.c by tests/test_guided_stub.py: one log line, "host call=<name>", per call with which a host thread waits for the
 * device or copies or fills memory, in the same log as fakehip.c's launch lines (FAKEHIP_LOG), so that a test can see that nothing of the kind
 * happens between two launches. Every call is passed on to the next library (fakehip.c). */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

static void note(const char* name) {
    const char* path = getenv("FAKEHIP_LOG");
    FILE* f = path ? fopen(path, "a") : NULL;
    if (f) { fprintf(f, "host call=%s\n", name); fclose(f); }
}
#define NEXT(type, name) ((type)dlsym(RTLD_NEXT, name))

int hipStreamSynchronize(void* s) { note("hipStreamSynchronize"); return NEXT(int (*)(void*), "hipStreamSynchronize")(s); }
int hipDeviceSynchronize(void) { note("hipDeviceSynchronize"); return NEXT(int (*)(void), "hipDeviceSynchronize")(); }
int hipEventSynchronize(void* e) { note("hipEventSynchronize"); return NEXT(int (*)(void*), "hipEventSynchronize")(e); }
int hipMemcpy(void* d, const void* s, size_t n, int kind) { note("hipMemcpy"); return NEXT(int (*)(void*, const void*, size_t, int), "hipMemcpy")(d, s, n, kind); }
int hipMemcpyAsync(void* d, const void* s, size_t n, int kind, void* st) {
    note("hipMemcpyAsync");
    return NEXT(int (*)(void*, const void*, size_t, int, void*), "hipMemcpyAsync")(d, s, n, kind, st);
}
int hipMemset(void* d, int v, size_t n) { note("hipMemset"); return NEXT(int (*)(void*, int, size_t), "hipMemset")(d, v, n); }
int hipMemsetAsync(void* d, int v, size_t n, void* st) { note("hipMemsetAsync"); return NEXT(int (*)(void*, int, size_t, void*), "hipMemsetAsync")(d, v, n, st); }
