// Shared by the library's translation units, not part of the public ABI (include/hftlob.h).
#ifndef HFTLOB_INTERNAL_H
#define HFTLOB_INTERNAL_H

// Records msg as the calling thread's hftlob_last_error() text and returns code
// (defined next to hftlob_last_error in hftlob.hip's main translation unit).
__attribute__((visibility("hidden"))) int hftlob_fail(int code, const char* msg);

#endif
