// TEST INFRASTRUCTURE ONLY -- host stand-in for <glm/glm.hpp>, written for this repository.
//
// Only the subset the reference's host sources use: vec3 with component arithmetic, dot, cross,
// length, normalize, component-wise min / max, scalar clamp and radians.  Each expression is
// spelled the way the GLM documentation defines the function for scalar (non-SIMD) floats, so the
// rounding sequence is the one a GLM build has: dot sums x, y, z products left to right,
// normalize multiplies by 1 / sqrt(dot(v, v)), a vector divided by a scalar divides each component.
#pragma once
#include <cmath>

namespace glm {

struct vec3 {
    float x, y, z;
    vec3() : x(0.0f), y(0.0f), z(0.0f) {}
    explicit vec3(float s) : x(s), y(s), z(s) {}
    vec3(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
    float &operator[](int i){ return i == 0 ? x : (i == 1 ? y : z); }
    const float &operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
    vec3 &operator+=(const vec3 &b){ x += b.x; y += b.y; z += b.z; return *this; }
    vec3 &operator-=(const vec3 &b){ x -= b.x; y -= b.y; z -= b.z; return *this; }
    vec3 &operator*=(float s){ x *= s; y *= s; z *= s; return *this; }
    vec3 &operator/=(float s){ x /= s; y /= s; z /= s; return *this; }
};

inline vec3 operator+(const vec3 &a, const vec3 &b){ return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline vec3 operator-(const vec3 &a, const vec3 &b){ return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline vec3 operator-(const vec3 &a){ return vec3(-a.x, -a.y, -a.z); }
inline vec3 operator*(const vec3 &a, const vec3 &b){ return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline vec3 operator*(const vec3 &a, float s){ return vec3(a.x * s, a.y * s, a.z * s); }
inline vec3 operator*(float s, const vec3 &a){ return vec3(s * a.x, s * a.y, s * a.z); }
inline vec3 operator/(const vec3 &a, float s){ return vec3(a.x / s, a.y / s, a.z / s); }
inline bool operator==(const vec3 &a, const vec3 &b){ return a.x == b.x && a.y == b.y && a.z == b.z; }

inline float dot(const vec3 &a, const vec3 &b){ vec3 t = a * b; return t.x + t.y + t.z; }
inline vec3 cross(const vec3 &a, const vec3 &b){
    return vec3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y);
}
inline float length(const vec3 &a){ return std::sqrt(dot(a, a)); }
inline float inversesqrt(float v){ return 1.0f / std::sqrt(v); }
inline vec3 normalize(const vec3 &a){ return a * inversesqrt(dot(a, a)); }

inline float min(float a, float b){ return (b < a) ? b : a; }
inline float max(float a, float b){ return (a < b) ? b : a; }
inline vec3 min(const vec3 &a, const vec3 &b){ return vec3(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z)); }
inline vec3 max(const vec3 &a, const vec3 &b){ return vec3(max(a.x, b.x), max(a.y, b.y), max(a.z, b.z)); }
inline float clamp(float v, float lo, float hi){ return min(max(v, lo), hi); }
inline float radians(float deg){ return deg * 0.01745329251994329576923690768489f; }
inline float degrees(float rad){ return rad * 57.295779513082320876798154814105f; }

} // namespace glm
