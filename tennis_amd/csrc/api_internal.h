// What the handles of api.hip and encoder.hip share on the host: the device allocations of a handle and the lookup of its
// parameters by name.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "common.h"

struct DevPool {  // owns device allocations of one handle
  std::vector<void *> ptrs;
  size_t bytes = 0;
  bool failed = false;
  void *alloc(size_t n) {
    void *p = nullptr;
    if (hipMalloc(&p, n ? n : 16) != hipSuccess) { failed = true; return nullptr; }
    ptrs.push_back(p);
    bytes += n;
    return p;
  }
  template <typename T>
  T *upload(const std::vector<T> &h) {
    T *d = (T *)alloc(h.size() * sizeof(T));
    if (d && hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { failed = true; return nullptr; }
    return d;
  }
  void release() {
    for (void *p : ptrs) (void)hipFree(p);
    ptrs.clear();
  }
};

struct ParamMap {
  std::map<std::string, const tn_param *> m;
  ParamMap(const tn_param *p, int n) {
    for (int i = 0; i < n; ++i) m[p[i].name] = &p[i];
  }
  const float *get(const std::string &name, int64_t numel) const {
    auto it = m.find(name);
    if (it == m.end()) {
      tn_set_error("missing parameter: " + name);
      return nullptr;
    }
    if (it->second->numel != numel) {
      tn_set_error("parameter " + name + " has " + std::to_string(it->second->numel) + " elements, expected " +
                   std::to_string(numel));
      return nullptr;
    }
    return it->second->data_host;
  }
};
