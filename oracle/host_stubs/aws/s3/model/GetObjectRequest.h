// TEST INFRASTRUCTURE: empty stand-in; the worker stages under test call nothing of the AWS SDK.
#pragma once
