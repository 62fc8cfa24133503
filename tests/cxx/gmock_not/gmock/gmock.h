// <gmock/gmock.h> for the reference's test/BDHI/DPStokes/dpstokes_test.cu, which uses ::testing::Not(::testing::DoubleNear(...)): the
// matchers of tests/cxx/gtest_lite/gtest/gtest.h plus Not.  Own code (no GoogleTest source).  This directory comes before gtest_lite on
// that program's include path (examples/Makefile), so the other programs' <gmock/gmock.h> stays as it is.
#pragma once
#include "../../gtest_lite/gtest/gtest.h"
namespace testing {
template <class M> class NotMatcher {
  M inner;
public:
  explicit NotMatcher(const M &m) : inner(m) {}
  template <class V> bool Matches(const V &v) const { return !inner.Matches(v); }
  std::string Describe() const { return "not (" + inner.Describe() + ")"; }
};
template <class M> inline NotMatcher<M> Not(const M &m) { return NotMatcher<M>(m); }
}  // namespace testing
