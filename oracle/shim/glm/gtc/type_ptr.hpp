// TEST INFRASTRUCTURE ONLY -- host stand-in for <glm/gtc/type_ptr.hpp>: the reference includes it but the pinned
// sources use nothing from it.
#pragma once
#include <glm/glm.hpp>
